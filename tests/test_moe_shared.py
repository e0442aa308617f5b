"""The complete slot list in the route launch: petit_moe_route_ex / petit_moe_route_align_ex (moe_route / moe_route_align / fp4_moe_routed with
expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits; include/petit_amd.h "The complete slot list in the route launch").

`route_ex_np` restates the definition on test_moe_route's `route_np`: slots 0 .. topk-1 are route_np's selection and float64 weights with the
ids sent through the map (a value outside [0, L) becomes -1; the weights are those of the GLOBAL selection), slots topk + s are the shared
experts: id L + s, weight shared_weight, times the float64 sigmoid of the gate logit when one is given.

Bounds (u = 2^-24).  An ungated shared weight is float32(shared_weight) exactly.  A gated one is the route's fp32 sigmoid (4 u: expf 2 u,
the add 1 u, the divide 1 u) times shared_weight (1 u): 5 u relative to the float64 statement on the same logits.  Routed weights keep
test_moe_route's derived bounds (`weight_bound_u`) and are compared BITWISE with the unmapped / unshared call of the same logits.

The layer tests compare fp4_moe_routed bit for bit with fp4_moe_fused / fp4_moe_native fed the statement's ids.  The routed weights handed to
those layers are the device's float32 weights, after they have been checked against the statement under the derived bound: the statement's
float64 weights are not float32 values, so "bit for bit" on the layer's output is only defined for float32 weights (the shared slots'
weights ARE the statement's, bitwise).

Measured on the MI355X (profiles/moe_shared.md): the largest error of a gated shared weight in these tests, in units of u.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_moe import _hints, _layer_ref, _make_layer
from test_moe_fused import align_np
from test_moe_route import _record, route_np, weight_bound_u, weights_np

DEV = "cuda"
U = 2.0 ** -24
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DEEPSEEK = dict(scoring="sigmoid", renormalize=True, n_group=8, topk_group=4, routed_scaling_factor=2.5)


# --- the definition, restated in numpy -------------------------------------------------------------------------------------------------

def route_ex_np(logits, topk, expert_map=None, num_local_experts=None, num_shared=0, shared_weight=1.0, shared_gate_logits=None, **routing):
    """(float64 weights [T, topk + S], int32 ids [T, topk + S], float32 keys [T, E]) of the _ex definition, on route_np."""
    w, g, keys = route_np(logits, topk, **routing)
    T, E = logits.shape
    L = E if num_local_experts is None else int(num_local_experts)
    ids = g.astype(np.int64)
    if expert_map is not None:
        m = np.asarray(expert_map, np.int64)[ids]
        ids = np.where((m >= 0) & (m < L), m, -1)
    S = int(num_shared)
    sw = np.full((T, S), float(np.float32(shared_weight)), np.float64)
    if shared_gate_logits is not None:
        with np.errstate(over="ignore"):
            sw = sw / (1.0 + np.exp(-shared_gate_logits.astype(np.float64)))
    shared_ids = np.broadcast_to(L + np.arange(S, dtype=np.int64), (T, S))
    return np.concatenate([w, sw], axis=1), np.concatenate([ids, shared_ids], axis=1).astype(np.int32), keys


def quarter_map(E):
    """A map that keeps a contiguous quarter of the experts (the second one): (map int32 [E], L)."""
    L = max(1, E // 4)
    g = np.arange(E)
    return np.where((g >= L) & (g < 2 * L), g - L, -1).astype(np.int32), L


def hostile_map(E, L, seed):
    """A map holding values outside [0, L) on both sides (not only -1): those ids must come out as -1."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-3, L + 4, E).astype(np.int32)
    m[0], m[-1] = -2147483648, 2147483647
    return m


# --- without a GPU ----------------------------------------------------------------------------------------------------------------------

def test_route_ex_abi_refusals_without_a_gpu():
    from petit_kernel import _lib
    lib = _lib.lib
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    shape, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    F32, SOFT, SIG = _lib.PETIT_DTYPE_FP32, _lib.PETIT_ROUTE_SOFTMAX, _lib.PETIT_ROUTE_SIGMOID
    MAXK, MAXE = _lib.PETIT_MOE_MAX_TOPK, _lib.PETIT_MOE_MAX_EXPERTS

    def desc(scoring=SOFT, renorm=1, n_group=0, topk_group=0, scale=0.0, bias=None):
        return _lib.RouteDesc(scoring, renorm, n_group, topk_group, scale, bias)

    def slots(emap=None, L=0, S=0, sw=0.0, gate=None):
        return _lib.RouteSlots(emap, L, S, sw, gate)

    def route(T=4, E=8, topk=2, d=None, sl=None, dtype=F32, logits=p, ids=p, w=p, keys=None):
        return lib.petit_moe_route_ex(logits, dtype, T, E, topk, C.byref(d) if d is not None else None, C.byref(sl) if sl is not None else None,
                                      ids, w, keys, None)

    def route_align(T=4, E=8, topk=2, d=None, sl=None, dtype=F32, logits=p, ids=p, w=p, off=p, sp=p, ti=p, ws=p):
        return lib.petit_moe_route_align_ex(logits, dtype, T, E, topk, C.byref(d) if d is not None else None,
                                            C.byref(sl) if sl is not None else None, ids, w, None, off, sp, ti, ws, None)

    for fn in (route, route_align):
        for sl in (None, slots(), slots(S=1), slots(emap=p, L=4, S=2)):
            # everything petit_moe_route refuses
            assert fn(topk=0, sl=sl) == shape
            assert fn(E=8, topk=9, sl=sl) == shape
            assert fn(E=256, topk=MAXK + 1, sl=sl) == shape
            assert fn(E=0, sl=sl) == shape and fn(E=MAXE + 1, sl=sl) == shape
            assert fn(T=1 << 27, E=64, topk=16, sl=sl) == shape
            assert fn(logits=None, sl=sl) == shape and fn(ids=None, sl=sl) == shape and fn(w=None, sl=sl) == shape
            assert fn(dtype=_lib.CXX_DTYPE_FP4_E2M1, sl=sl) == bad and fn(dtype=0, sl=sl) == bad
            assert fn(d=desc(scoring=2), sl=sl) == bad and fn(d=desc(scoring=-1), sl=sl) == bad
            assert fn(E=8, d=desc(SIG, n_group=3, topk_group=1), sl=sl) == shape
            assert fn(E=8, d=desc(SIG, n_group=4, topk_group=0), sl=sl) == shape
            assert fn(E=8, d=desc(SIG, n_group=4, topk_group=5), sl=sl) == shape
            assert fn(E=8, d=desc(SIG, n_group=1, topk_group=2), sl=sl) == shape
            assert fn(E=8, topk=5, d=desc(SIG, n_group=4, topk_group=2), sl=sl) == shape
            assert fn(E=8, topk=1, d=desc(SIG, n_group=8, topk_group=2), sl=sl) == shape
            assert fn(E=8, d=desc(SOFT, n_group=2, topk_group=1), sl=sl) == shape
            assert fn(E=8, d=desc(SOFT, bias=p), sl=sl) == shape
        # the slot list's own refusals
        assert fn(E=256, topk=MAXK, sl=slots(S=1)) == shape                                # topk + S > PETIT_MOE_MAX_TOPK
        assert fn(E=256, topk=8, sl=slots(S=MAXK - 7)) == shape
        assert fn(E=MAXE, topk=8, sl=slots(S=1)) == shape                                  # L + S > PETIT_MOE_MAX_EXPERTS
        assert fn(E=MAXE, topk=8, sl=slots(emap=p, L=MAXE - 1, S=2)) == shape
        assert fn(E=8, sl=slots(emap=p, L=9)) == shape                                     # L > num_experts
        assert fn(E=8, sl=slots(L=4)) == shape and fn(E=8, sl=slots(L=4, S=1)) == shape    # L != num_experts without a map
        assert fn(T=1 << 27, E=64, topk=15, sl=slots(S=1)) == shape                        # T * (topk + S) >= 2^31
        assert fn(sl=slots(gate=p)) == shape and fn(sl=slots(emap=p, L=4, gate=p)) == shape  # gate logits with S == 0
    assert route_align(sl=slots(S=1), off=None) == shape and route_align(sl=slots(S=1), sp=None) == shape
    assert route_align(T=114, E=256, topk=8, sl=slots(S=1), ws=None) == shape              # 1026 entries: several chunks need the workspace
    assert route_align(T=0, sl=slots(S=1), off=None) == shape
    # accepted without a launch: nothing to do
    for sl in (None, slots(), slots(L=8), slots(S=1, sw=0.5), slots(S=2, gate=p), slots(emap=p, L=4, S=1), slots(emap=p, S=1),
               slots(emap=p, L=8, S=MAXK - 2)):
        assert route(T=0, sl=sl, logits=None, ids=None, w=None) == ok
    assert route(T=0, E=MAXE, topk=8, sl=slots(emap=p, L=MAXE - 1, S=1), logits=None, ids=None, w=None) == ok
    # the workspace is the align's on T * (topk + S) entries over L + S experts
    wsb, awb = lib.petit_moe_route_align_ex_workspace_bytes, lib.petit_moe_align_workspace_bytes
    for T, topk, E in ((1, 8, 256), (113, 8, 256), (114, 8, 256), (128, 8, 256), (4096, 8, 1000), (4, 0, 8), (1000, 32, 384)):
        assert wsb(T, topk, E, None) == awb(T, topk, E) == lib.petit_moe_route_align_workspace_bytes(T, topk, E)
        assert wsb(T, topk, E, C.byref(slots())) == awb(T, topk, E)
        assert wsb(T, topk, E, C.byref(slots(S=1))) == awb(T, topk + 1, E + 1)
        assert wsb(T, topk, E, C.byref(slots(emap=p, L=E // 4, S=2))) == awb(T, topk + 2, E // 4 + 2)
    assert wsb(114, 8, 256, C.byref(slots(S=1))) > 0 and wsb(113, 8, 256, C.byref(slots(S=1))) == 0


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("return_keys", [False, True])
def test_route_ex_ops_meta_shapes(dt, return_keys):
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    ops = torch.ops.petit_kernel
    T, E, topk = 6, 256, 8
    logits = torch.empty(T, E, dtype=TORCH_DT[dt], device="meta")
    bias = torch.empty(E, dtype=torch.float32, device="meta")
    emap = torch.empty(E, dtype=torch.int32, device="meta")
    for L, S, kw in ((E, 0, {}), (E, 1, dict(num_shared=1)), (64, 2, dict(expert_map=emap, num_local_experts=64, num_shared=2,
                                                                         shared_gate_logits=torch.empty(T, 2, dtype=TORCH_DT[dt], device="meta")))):
        w, ids, keys = ops.moe_route_ex(logits, topk, 1, True, bias, 8, 4, 2.5, return_keys, **kw)
        assert w.shape == (T, topk + S) and w.dtype == torch.float32 and ids.shape == (T, topk + S) and ids.dtype == torch.int32
        assert w.device.type == "meta" and keys.dtype == torch.float32 and tuple(keys.shape) == ((T, E) if return_keys else (0,))
        w, ids, sp, off, ti, keys = ops.moe_route_align_ex(logits, topk, 0, True, None, 1, 1, 1.0, return_keys, **kw)
        assert w.shape == (T, topk + S) and w.dtype == torch.float32 and ids.shape == (T, topk + S) and ids.dtype == torch.int32
        assert sp.shape == (T * (topk + S),) and ti.shape == (T * (topk + S),) and off.shape == (L + S + 1,)
        assert sp.dtype == off.dtype == ti.dtype == torch.int32
        assert tuple(keys.shape) == ((T, E) if return_keys else (0,)) and keys.dtype == torch.float32


def test_route_ex_np_by_hand():
    """Two tokens, E = 4, top-2, softmax with renormalize: the selection is (1, 3) and (0, 2)."""
    logits = np.array([[0.0, 2.0, -1.0, 1.0], [3.0, 0.0, 3.0 - np.log(3.0), -2.0]], np.float32)
    e = np.exp(1.0)
    want_w = np.array([[e / (1 + e), 1 / (1 + e)], [0.75, 0.25]])
    w, ids, keys = route_ex_np(logits, 2)
    assert ids.tolist() == [[1, 3], [0, 2]] and np.allclose(w, want_w, rtol=1e-6, atol=0) and np.array_equal(keys, logits)
    # a map: experts 2, 3 are local experts 0, 1; the weights stay those of the global selection
    w, ids, _ = route_ex_np(logits, 2, expert_map=[-1, -1, 0, 1], num_local_experts=2)
    assert ids.tolist() == [[-1, 1], [-1, 0]] and np.allclose(w, want_w, rtol=1e-6, atol=0)
    # values outside [0, L) on either side are -1
    w, ids, _ = route_ex_np(logits, 2, expert_map=[2, 1, -7, 0], num_local_experts=2)
    assert ids.tolist() == [[1, 0], [-1, -1]]
    # two shared slots after the routed ones: ids L, L + 1; the weight is shared_weight, untouched by the scaling factor
    w, ids, _ = route_ex_np(logits, 2, expert_map=[-1, -1, 0, 1], num_local_experts=2, num_shared=2, shared_weight=0.5, routed_scaling_factor=2.0)
    assert ids.tolist() == [[-1, 1, 2, 3], [-1, 0, 2, 3]]
    assert np.allclose(w[:, :2], 2.0 * want_w, rtol=1e-6, atol=0) and (w[:, 2:] == 0.5).all()
    # gated: shared_weight * sigmoid(gate)
    gate = np.array([[0.0], [np.log(3.0)]], np.float32)
    w, ids, _ = route_ex_np(logits, 2, num_shared=1, shared_weight=2.0, shared_gate_logits=gate)
    assert ids.tolist() == [[1, 3, 4], [0, 2, 4]] and np.allclose(w[:, 2], [1.0, 1.5], rtol=1e-6, atol=0)


def test_package_takes_the_slot_list_arguments():
    import inspect

    import petit_kernel as pk
    for fn in (pk.moe_route, pk.moe_route_align):
        ps = inspect.signature(fn).parameters
        for name, default in (("expert_map", None), ("num_local_experts", None), ("num_shared", 0), ("shared_weight", 1.0),
                              ("shared_gate_logits", None)):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY and ps[name].default == default


# --- on the GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _f32(t):
    return t.detach().float().cpu().numpy()


def _i32(t):
    return t.view(torch.int32)


def _np_routing(routing):
    return {k: (_f32(v) if k == "bias" else v) for k, v in routing.items()}


def _bias(E, seed):
    return torch.randn(E, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["softmax", "sigmoid", "grouped"])
def test_defaults_are_the_plain_route_bit_for_bit(pk, case):
    """moe_route / moe_route_align with every new argument at its default equal the _ex entries with null slots (the C ABI with a null
    pointer), with zero-initialised slots, and the _ex ops of both layers with their defaults: ids, weights, keys, and the align."""
    from petit_kernel import _lib, compiled, ops
    E, topk = (60, 4) if case == "softmax" else (256, 8)
    routing = {"softmax": dict(scoring="softmax", renormalize=False), "sigmoid": dict(scoring="sigmoid", renormalize=True, bias=_bias(E, 1)),
               "grouped": dict(DEEPSEEK, bias=_bias(E, 2))}[case]
    g = torch.Generator(device=DEV).manual_seed(11)
    for T, dt in ((1, "f32"), (37, "bf16"), (200, "f16")):
        logits = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
        w, ids, keys = pk.moe_route(logits, topk, return_keys=True, **routing)
        aw, aids, sp, off, ti, akeys = pk.moe_route_align(logits, topk, return_keys=True, **routing)
        assert ids.shape == (T, topk) and torch.equal(aids, ids) and torch.equal(_i32(aw), _i32(w)) and torch.equal(_i32(akeys), _i32(keys))
        for layer in (compiled, ops):
            xw, xids, xkeys = layer.moe_route_ex(logits, topk, return_keys=True, **routing)
            assert torch.equal(xids, ids) and torch.equal(_i32(xw), _i32(w)) and torch.equal(_i32(xkeys), _i32(keys))
            xw, xids, xsp, xoff, xti, xkeys = layer.moe_route_align_ex(logits, topk, return_keys=True, **routing)
            assert torch.equal(xids, ids) and torch.equal(_i32(xw), _i32(w)) and torch.equal(_i32(xkeys), _i32(keys))
            assert torch.equal(xsp, sp) and torch.equal(xoff, off) and torch.equal(xti, ti)
        # the C ABI: a null slot list, and a zero-initialised one
        desc = ops._route_desc(routing["scoring"], routing["renormalize"], routing.get("bias"), routing.get("n_group", 1),
                               routing.get("topk_group", 1), routing.get("routed_scaling_factor", 1.0))
        for sl in (None, C.byref(_lib.RouteSlots())):
            cw, cids, ckeys = torch.empty_like(w), torch.empty_like(ids), torch.empty_like(keys)
            rc = _lib.lib.petit_moe_route_ex(logits.data_ptr(), ops._LOGIT_DTYPES[logits.dtype], T, E, topk, C.byref(desc), sl, cids.data_ptr(),
                                             cw.data_ptr(), ckeys.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == _lib.PETIT_OK
            assert torch.equal(cids, ids) and torch.equal(_i32(cw), _i32(w)) and torch.equal(_i32(ckeys), _i32(keys))


MAP_CASES = {  # E: (topk, routing) -- DeepSeek-V3's grouping needs E % 8 == 0 and groups of >= 2 experts: it rides on E = 256
    8: (2, dict(scoring="softmax", renormalize=True)),
    65: (8, dict(scoring="sigmoid", renormalize=True, routed_scaling_factor=2.5, bias=True)),
    256: (8, dict(DEEPSEEK, bias=True)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("E", sorted(MAP_CASES))
def test_expert_map(pk, E, T):
    """ids == where(0 <= map[g] < L, map[g], -1) with g the statement's selection; the weights are bitwise those of the unmapped call (the
    renormalisation runs over the global selection); keys_out is unchanged."""
    topk, routing = MAP_CASES[E]
    routing = dict(routing)
    if routing.get("bias"):
        routing["bias"] = _bias(E, E)
    else:
        routing.pop("bias", None)
    g = torch.Generator(device=DEV).manual_seed(100 * E + T)
    qmap, L = quarter_map(E)
    for n, (emap, dt) in enumerate(((qmap, "f32"), (hostile_map(E, L, E + T), "bf16"), (qmap, "f16"))):
        logits = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
        w0, ids0, keys0 = pk.moe_route(logits, topk, return_keys=True, **routing)
        _, want_ids, _ = route_ex_np(_f32(logits), topk, expert_map=emap, num_local_experts=L, **_np_routing(routing))
        emap_d = torch.from_numpy(emap).to(DEV)
        w, ids, keys = pk.moe_route(logits, topk, return_keys=True, expert_map=emap_d, num_local_experts=L, **routing)
        assert ids.dtype == torch.int32 and ids.shape == (T, topk)
        g_np = ids0.cpu().numpy().astype(np.int64)
        assert np.array_equal(g_np, route_np(_f32(logits), topk, **_np_routing(routing))[1]), "the unmapped selection is not the statement's"
        m = emap.astype(np.int64)[g_np]
        assert np.array_equal(ids.cpu().numpy(), np.where((m >= 0) & (m < L), m, -1))
        assert np.array_equal(ids.cpu().numpy(), want_ids)
        assert torch.equal(_i32(w), _i32(w0)) and torch.equal(_i32(keys), _i32(keys0))
        if n == 0:
            assert (ids.cpu().numpy() == -1).any() or T == 1
        # the same through the one-launch form
        aw, aids, sp, off, ti = pk.moe_route_align(logits, topk, expert_map=emap_d, num_local_experts=L, **routing)
        assert torch.equal(aids, ids) and torch.equal(_i32(aw), _i32(w))
        rsp, roff, rti = align_np(want_ids, L)
        assert np.array_equal(sp.cpu().numpy(), rsp) and np.array_equal(off.cpu().numpy(), roff) and np.array_equal(ti.cpu().numpy(), rti)
    # a map without num_local_experts: L = E
    ident = torch.arange(E, dtype=torch.int32, device=DEV).flip(0).contiguous()
    w, ids = pk.moe_route(logits, topk, expert_map=ident, **routing)
    assert torch.equal(ids, E - 1 - ids0) and torch.equal(_i32(w), _i32(w0))


SHARED_CASES = [  # (E, topk, S, T, routing)
    (8, 2, 1, 5, dict(scoring="softmax", renormalize=True)),
    (65, 8, 2, 33, dict(scoring="sigmoid", renormalize=False)),
    (256, 8, 1, 130, dict(DEEPSEEK, bias=True)),
    (256, 8, 2, 7, dict(DEEPSEEK, bias=True)),
    (64, 62, 2, 17, dict(scoring="softmax", renormalize=True)),          # topk + S = PETIT_MOE_MAX_TOPK: every lane holds a slot
    (64, 62, 2, 3, dict(scoring="sigmoid", renormalize=True)),
    (1000, 8, 2, 5, dict(scoring="sigmoid", renormalize=True, routed_scaling_factor=2.5, bias=True)),   # 16 keys per lane, both launch forms
]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", SHARED_CASES, ids=[f"E{c[0]}-top{c[1]}-S{c[2]}-T{c[3]}-{c[4]['scoring']}" for c in SHARED_CASES])
def test_shared_slots(pk, case, dt):
    """Slots topk + s: ids L + s; ungated weights are float32(shared_weight) bitwise, gated ones within 5 u of the float64 statement for gate
    logits in [-16, 16]; the routed slots are bitwise the plain call's (routed_scaling_factor does not reach the shared slots); with a map
    the shared ids follow the LOCAL experts.  Both launch forms."""
    E, topk, S, T, routing = case
    routing = dict(routing)
    if routing.pop("bias", None):
        routing["bias"] = _bias(E, 3)
    g = torch.Generator(device=DEV).manual_seed(E + topk + S + T)
    logits = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
    gate = ((torch.rand(T, S, device=DEV, generator=g) * 32 - 16)).to(TORCH_DT[dt])
    gate[0, 0], gate[-1, -1] = -16.0, 16.0
    w0, ids0 = pk.moe_route(logits, topk, **routing)
    qmap, L = quarter_map(E)
    for sw in (1.0, 0.3, 2.5):
        for emap, Lx in ((None, E), (qmap, L)):
            kw = dict(routing, num_shared=S, shared_weight=sw)
            if emap is not None:
                kw.update(expert_map=torch.from_numpy(emap).to(DEV), num_local_experts=Lx)
            np_kw = dict(_np_routing(routing), num_shared=S, shared_weight=sw, expert_map=emap, num_local_experts=Lx)
            for gated in (False, True):
                if gated:
                    kw["shared_gate_logits"], np_kw["shared_gate_logits"] = gate, _f32(gate)
                ref_w, ref_ids, _ = route_ex_np(_f32(logits), topk, **np_kw)
                for align in (False, True):
                    out = (pk.moe_route_align if align else pk.moe_route)(logits, topk, **kw)
                    w, ids = out[0], out[1]
                    assert w.shape == (T, topk + S) and ids.shape == (T, topk + S) and w.dtype == torch.float32 and ids.dtype == torch.int32
                    assert np.array_equal(ids.cpu().numpy(), ref_ids)
                    assert (ids[:, topk:].cpu() == Lx + torch.arange(S, dtype=torch.int32)).all()
                    assert torch.equal(_i32(w[:, :topk].contiguous()), _i32(w0))
                    got = w[:, topk:].cpu().numpy()
                    if not gated:
                        assert np.array_equal(got.view(np.uint32), np.full((T, S), sw, np.float32).view(np.uint32))
                    else:
                        ref = ref_w[:, topk:]
                        err = np.abs(got.astype(np.float64) - ref) / ref / U
                        print(f"gated shared weight E {E} S {S} T {T} {dt} weight {sw}: max error {err.max():.2f} u (bound 5 u)")
                        _record("shared gated", err.max())
                        assert (err <= 5.0).all(), f"gated shared weight error {err.max():.2f} u > 5 u"
                    if align:
                        rsp, roff, rti = align_np(ref_ids, Lx + S)
                        assert np.array_equal(out[2].cpu().numpy(), rsp) and np.array_equal(out[3].cpu().numpy(), roff)
                        assert np.array_equal(out[4].cpu().numpy(), rti)
    # the routed weights against the statement, under their derived bound (the layer tests lean on this)
    ref = weights_np(_f32(logits), ids0.cpu().numpy(), routing["scoring"], routing["renormalize"], routing.get("routed_scaling_factor", 1.0))
    bound = weight_bound_u(_f32(logits), ids0.cpu().numpy(), routing["scoring"], routing["renormalize"])
    assert bound <= 256.0 and (np.abs(w0.cpu().numpy() - ref) <= bound * U * ref).all()
    with pytest.raises(RuntimeError):
        pk.moe_route(logits, topk, shared_gate_logits=gate, **routing)                         # gate logits without shared experts
    with pytest.raises(RuntimeError):
        pk.moe_route(logits, topk, num_local_experts=L, **routing)                            # local experts without a map
    with pytest.raises(RuntimeError):
        pk.moe_route(logits, topk, num_shared=65 - topk, **routing)


@pytest.mark.gpu
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("T", [113, 114])
def test_route_align_with_shared_is_route_then_align(pk, T, mapped):
    """topk 8 + 1 shared slot: 1017 entries at T = 113 (ONE launch), 1026 at T = 114 (the route launch and the align's three).  Bit for bit
    moe_route (the grid form) followed by moe_align_device(ids, L + S); both layers agree; repeated calls repeat."""
    from petit_kernel import compiled, ops
    E, topk, S = 256, 8, 1
    routing = dict(DEEPSEEK, bias=_bias(E, 4))
    g = torch.Generator(device=DEV).manual_seed(T)
    logits = torch.randn(T, E, device=DEV, generator=g).bfloat16()
    gate = torch.randn(T, S, device=DEV, generator=g).bfloat16()
    kw = dict(routing, num_shared=S, shared_weight=0.75, shared_gate_logits=gate)
    L = E
    if mapped:
        emap, L = quarter_map(E)
        kw.update(expert_map=torch.from_numpy(emap).to(DEV), num_local_experts=L)
    w, ids, keys = pk.moe_route(logits, topk, return_keys=True, **kw)
    assert ids.shape == (T, topk + S) and (not mapped or (ids == -1).any())
    sp, off, ti = pk.moe_align_device(ids, L + S)
    rsp, roff, rti = align_np(ids.cpu().numpy(), L + S)
    assert np.array_equal(sp.cpu().numpy(), rsp) and np.array_equal(off.cpu().numpy(), roff) and np.array_equal(ti.cpu().numpy(), rti)
    assert int(off[-1]) - int(off[L]) == T                                                   # every token has its shared slot
    for layer in (pk, compiled, ops):
        fn = layer.moe_route_align if layer is pk else layer.moe_route_align_ex
        for _ in range(2):
            fw, fids, fsp, foff, fti, fkeys = fn(logits, topk, return_keys=True, **kw)
            assert torch.equal(fids, ids) and torch.equal(_i32(fw), _i32(w)) and torch.equal(_i32(fkeys), _i32(keys))
            assert foff.numel() == L + S + 1 and torch.equal(fsp, sp) and torch.equal(foff, off) and torch.equal(fti, ti)


# --- the layer --------------------------------------------------------------------------------------------------------------------------

E_ROUTED, TOPK, HID, INTER = 8, 2, 1024, 512                      # test_routed_layer_is_the_layer's shape, plus one shared expert
LAYER_ROUTING = dict(scoring="sigmoid", renormalize=True, n_group=4, topk_group=2, routed_scaling_factor=2.5)


def _bits(t):
    return t.view(torch.int16)


def _statement_routing(pk, logits, kw, np_kw):
    """The statement's ids and the float32 weights the layers are fed (module docstring): ids are route_ex_np's, exactly; the shared slots'
    weights are the statement's, bitwise; the routed slots' weights are the device's, checked against the statement under the derived bound."""
    w, ids = pk.moe_route(logits, TOPK, **kw)
    ref_w, ref_ids, _ = route_ex_np(_f32(logits), TOPK, **np_kw)
    assert np.array_equal(ids.cpu().numpy(), ref_ids)
    got = w.cpu().numpy()
    S = ref_ids.shape[1] - TOPK
    assert np.array_equal(got[:, TOPK:].view(np.uint32), ref_w[:, TOPK:].astype(np.float32).view(np.uint32))
    bound = weight_bound_u(_f32(logits), ref_ids[:, :TOPK], np_kw["scoring"], np_kw["renormalize"])   # (no map here: the ids are global)
    assert bound <= 256.0 and (np.abs(got[:, :TOPK] - ref_w[:, :TOPK]) <= bound * U * ref_w[:, :TOPK]).all()
    return torch.from_numpy(got).to(DEV), torch.from_numpy(ref_ids).to(DEV), ref_w, ref_ids, S


def _oracle_layer(x, w13, w2, ref_w, ref_ids):
    """The f64 layer on the statement's slots: unrouted (-1) slots contribute nothing."""
    keep = ref_ids >= 0
    return _layer_ref(x.cpu().view(torch.int16).numpy().view(np.uint16), w13, w2, np.where(keep, ref_w, 0.0), np.where(keep, ref_ids, 0))


def _rel_rms(out, ref):
    err = out.astype(np.float64) - ref
    return np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2))


def _dense_expert(pk, ex, e):
    n, k = ex.n, ex.k
    per_s = n * k // (16 if ex.kind == "nv" else 32)
    b = ex.b.view(-1)[e * n * k // 8:(e + 1) * n * k // 8].view(n // 16, 2 * k)
    s = ex.sp.view(-1)[e * per_s:(e + 1) * per_s]
    return b, (s.view(n, k // 16) if ex.kind == "nv" else s.view(n // 32, k)), ex.gsd[e:e + 1]


def _dense_rows(dense, a, b, s, gs, n, k, sid, **kw):
    """A dense call with kernel id `sid` on ALL rows of a.  A streaming kernel holds a fixed number of rows (the MoE launch hands it an
    expert's rows in blocks of that many), and the dense call refuses more: then the rows go in equal blocks of the largest size it takes.
    A row's result does not depend on the rows next to it, so this is still the dense call's value of every row.  Only the launcher's own
    refusal of the row count (made before any launch) moves on to a smaller block; every other error ends the test."""
    T = a.shape[0]
    for rows in (T, 16, 8, 4, 2, 1):
        if rows > T:
            continue
        try:
            return torch.cat([dense(a[i:i + rows].contiguous(), b, s, gs, min(rows, T - i), n, k, sid, **kw) for i in range(0, T, rows)])
        except RuntimeError as exc:
            if "Incompatible problem shape" not in str(exc):   # the launcher's refusal before any launch; anything else is a failure
                raise
    raise AssertionError(f"the dense call refuses id {sid:#x} at every row count")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [5, 33])
@pytest.mark.parametrize("kind", ["nvfp4", "mxfp4"])
def test_routed_layer_with_a_shared_expert_exact_path(pk, kind, T):
    EA = E_ROUTED + 1
    w13, w2 = _make_layer(pk, kind[:2], EA, HID, INTER, 91)
    g = torch.Generator(device=DEV).manual_seed(T)
    x = torch.randn(T, HID, device=DEV, generator=g).bfloat16()
    logits = torch.randn(T, E_ROUTED, device=DEV, generator=g).bfloat16()
    routing = dict(LAYER_ROUTING, bias=_bias(E_ROUTED, 5))
    kw = dict(routing, num_shared=1)
    wts = (w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd)
    got = pk.fp4_moe_routed(x, logits, *wts, TOPK, kind, **kw)
    assert got.shape == (T, HID) and got.dtype == torch.bfloat16
    # (a) fp4_moe_fused on the statement's slots
    tw, tid, ref_w, ref_ids, S = _statement_routing(pk, logits, kw, dict(_np_routing(routing), num_shared=1))
    assert S == 1 and (ref_ids[:, TOPK] == E_ROUTED).all() and (ref_w[:, TOPK] == 1.0).all()
    fused = pk.fp4_moe_fused(x, *wts, tw, tid, kind)
    assert torch.equal(_bits(got), _bits(fused))
    # (b) the shared expert's slot rows before the combine are dense calls on all token rows, with the ids the MoE launches resolve to
    mul = pk.mul_nvfp4_a16_moe_indexed if kind == "nvfp4" else pk.mul_mxfp4_a16_moe_indexed
    dense = pk.mul_nvfp4_a16 if kind == "nvfp4" else pk.mul_mxfp4_a16
    rw, rids, sp, off, ti = pk.moe_route_align(logits, TOPK, **kw)
    slots, m = TOPK + 1, T * (TOPK + 1)
    h = mul(x, w13.b, w13.sp, w13.gsd, off, m, 2 * INTER, HID, EA, a_row_index=ti, activation="silu_mul")
    y = mul(h, w2.b, w2.sp, w2.gsd, off, m, HID, INTER, EA, c_row_index=sp, c_rows=m)
    assert torch.equal(_bits(pk.moe_combine(y, rw, rids, EA)), _bits(got))
    hints = _hints(pk, kind[:2], True)
    sid13 = pk.moe_resolve_solution(hints, EA, m, 2 * INTER, HID, -1, "silu_mul")
    sid2 = pk.moe_resolve_solution(hints, EA, m, HID, INTER, -1)
    assert sid13 and sid2
    dh = _dense_rows(dense, x, *_dense_expert(pk, w13, E_ROUTED), 2 * INTER, HID, sid13, activation="silu_mul")
    dy = _dense_rows(dense, dh, *_dense_expert(pk, w2, E_ROUTED), HID, INTER, sid2)
    shared_rows = y.view(T, slots, HID)[:, TOPK, :].contiguous()
    assert torch.equal(_bits(shared_rows), _bits(dy)), "the shared expert's slot rows differ from the dense calls"
    # (c) the oracle composition: routed layer + shared MLP, f64 (test_fp4_moe_fused_end_to_end's budget)
    ref = _oracle_layer(x, w13, w2, ref_w, ref_ids)
    rel = _rel_rms(got.float().cpu().numpy(), ref)
    print(f"{kind} T {T}: rms error / output rms {rel:.3e} (budget 1e-2)")
    assert rel <= 1e-2
    # the layer names its expert count: the stacks must hold the routed experts and the shared one
    with pytest.raises(RuntimeError):
        pk.fp4_moe_routed(x, logits, *wts, TOPK, kind, **routing)
    with pytest.raises(RuntimeError):
        pk.fp4_moe_routed(x, logits, *wts, TOPK, kind, **dict(routing, num_shared=2))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [5, 33])
@pytest.mark.parametrize("kind", ["nvfp4", "mxfp4"])
def test_routed_layer_with_a_shared_expert_native_path(pk, kind, T):
    from test_moe_native import _native_layer
    EA = E_ROUTED + 1
    w13, w2, b13, s13, b2, s2 = _native_layer(pk, kind[:2], EA, HID, INTER, 92)
    g = torch.Generator(device=DEV).manual_seed(40 + T)
    x = torch.randn(T, HID, device=DEV, generator=g).bfloat16()
    logits = torch.randn(T, E_ROUTED, device=DEV, generator=g).float()
    gate = torch.randn(T, 1, device=DEV, generator=g).float()
    routing = dict(LAYER_ROUTING, bias=_bias(E_ROUTED, 6))
    kw = dict(routing, num_shared=1, shared_gate_logits=gate)
    got = pk.fp4_moe_routed(x, logits, b13, s13, w13.gsd, b2, s2, w2.gsd, TOPK, kind, path="native", activations="mxfp8", **kw)
    w, ids = pk.moe_route(logits, TOPK, **kw)
    ref_w, ref_ids, _ = route_ex_np(_f32(logits), TOPK, **dict(_np_routing(routing), num_shared=1, shared_gate_logits=_f32(gate)))
    assert np.array_equal(ids.cpu().numpy(), ref_ids)
    bound = weight_bound_u(_f32(logits), ref_ids[:, :TOPK], routing["scoring"], routing["renormalize"])
    assert bound <= 256.0 and (np.abs(w.cpu().numpy()[:, :TOPK] - ref_w[:, :TOPK]) <= bound * U * ref_w[:, :TOPK]).all()   # the gated shared slot: 5 u
    assert (np.abs(w.cpu().numpy()[:, TOPK:] - ref_w[:, TOPK:]) <= 5 * U * ref_w[:, TOPK:]).all()
    native = pk.fp4_moe_native(x, b13, s13, w13.gsd, b2, s2, w2.gsd, w, torch.from_numpy(ref_ids).to(DEV), kind=kind, activations="mxfp8")
    assert got.shape == (T, HID) and torch.equal(_bits(got), _bits(native))


def _sub_stack(ex, experts):
    """The packed stacks of a subset of ex's experts (an expert's packed tensors are contiguous in the stack)."""
    n, k = ex.n, ex.k
    per_b, per_s = n * k // 8, n * k // 16
    b = torch.cat([ex.b.view(-1)[e * per_b:(e + 1) * per_b] for e in experts]).view(len(experts) * n // 16, 2 * k)
    s = torch.cat([ex.sp.view(-1)[e * per_s:(e + 1) * per_s] for e in experts]).view(len(experts) * n, k // 16)
    return b, s, ex.gsd[torch.tensor(experts, device=DEV)].contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [5, 33])
def test_expert_parallel_composition(pk, T):
    """Two ranks with complementary maps over the same logits, the (replicated) shared expert on rank 0 only: the fp32 sum of the ranks'
    outputs is within the fused layer's budget of the unsharded layer's oracle."""
    EA = E_ROUTED + 1
    w13, w2 = _make_layer(pk, "nv", EA, HID, INTER, 93)
    g = torch.Generator(device=DEV).manual_seed(80 + T)
    x = torch.randn(T, HID, device=DEV, generator=g).bfloat16()
    logits = torch.randn(T, E_ROUTED, device=DEV, generator=g).bfloat16()
    routing = dict(LAYER_ROUTING, bias=_bias(E_ROUTED, 7))
    rank_experts = ([0, 2, 5, 7], [1, 3, 4, 6])
    total = torch.zeros(T, HID, dtype=torch.float32, device=DEV)
    seen = np.zeros((T, TOPK), int)
    for rank, experts in enumerate(rank_experts):
        emap = np.full(E_ROUTED, -1, np.int32)
        emap[experts] = np.arange(len(experts))
        S = 1 if rank == 0 else 0
        stack = experts + ([E_ROUTED] if S else [])
        b13, s13, gs13 = _sub_stack(w13, stack)
        b2, s2, gs2 = _sub_stack(w2, stack)
        kw = dict(routing, expert_map=torch.from_numpy(emap).to(DEV), num_local_experts=len(experts), num_shared=S)
        out = pk.fp4_moe_routed(x, logits, b13, s13, gs13, b2, s2, gs2, TOPK, "nvfp4", **kw)
        total += out.float()
        _, ids = pk.moe_route(logits, TOPK, **kw)
        seen += (ids[:, :TOPK].cpu().numpy() >= 0)
    assert (seen == 1).all()                                                                 # every routed slot is local to exactly one rank
    ref_w, ref_ids, _ = route_ex_np(_f32(logits), TOPK, **dict(_np_routing(routing), num_shared=1))
    ref = _oracle_layer(x, w13, w2, ref_w, ref_ids)
    rel = _rel_rms(total.cpu().numpy(), ref)
    print(f"EP, 2 ranks, T {T}: rms error / output rms {rel:.3e} (budget 1e-2)")
    assert rel <= 1e-2


@pytest.mark.gpu
def test_routed_layer_with_slots_graph_replay_with_changing_logits(pk):
    """fp4_moe_routed with num_shared=1 and an expert map captured once on one stream (no parallel branches), replayed with three different
    logit tensors copied into the captured input: each replay equals the eager call."""
    T = 16
    experts = [1, 2, 4, 7, 3]                                                                # 5 local routed experts, then the shared one
    full13, full2 = _make_layer(pk, "nv", E_ROUTED + 1, HID, INTER, 94)
    b13, s13, gs13 = _sub_stack(full13, experts + [E_ROUTED])
    b2, s2, gs2 = _sub_stack(full2, experts + [E_ROUTED])
    emap = np.full(E_ROUTED, -1, np.int32)
    emap[experts] = np.arange(len(experts))
    g = torch.Generator(device=DEV).manual_seed(8)
    kw = dict(LAYER_ROUTING, bias=_bias(E_ROUTED, 8), expert_map=torch.from_numpy(emap).to(DEV), num_local_experts=len(experts), num_shared=1,
              shared_weight=0.5)

    def layer(xx, ll):
        return pk.fp4_moe_routed(xx, ll, b13, s13, gs13, b2, s2, gs2, TOPK, "nvfp4", **kw)

    sx, sl = torch.randn(T, HID, device=DEV, generator=g).bfloat16(), torch.randn(T, E_ROUTED, device=DEV, generator=g).bfloat16()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(sx, sl)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = layer(sx, sl)
    torch.cuda.synchronize()
    for i in range(3):
        xi = torch.randn(T, HID, device=DEV, generator=g).bfloat16()
        li = torch.randn(T, E_ROUTED, device=DEV, generator=g).bfloat16() if i < 2 else torch.zeros(T, E_ROUTED, device=DEV).bfloat16()
        sx.copy_(xi)
        sl.copy_(li)
        graph.replay()
        torch.cuda.synchronize()
        eager, again = layer(xi, li), layer(xi, li)
        torch.cuda.synchronize()
        assert torch.equal(_bits(eager), _bits(again))
        assert torch.equal(_bits(out), _bits(eager)), f"replay {i} differs from the eager call"

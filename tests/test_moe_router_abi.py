"""The router's GEMM (include/petit_amd.h "The router's GEMM") without a GPU: the symbols, every refusal that precedes a launch, the geometry
(S slices of L along K, functions of (E, K, a_type) alone), the workspace arithmetic, and the two operator layers' signatures."""
import ctypes as C
import inspect

import pytest

from petit_kernel import _lib

FP16, BF16 = _lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_BF16
OK, SHAPE, BAD = _lib.PETIT_OK, _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT
SYMBOLS = ("petit_moe_router_geometry", "petit_moe_router_slabs", "petit_moe_router_workspace_bytes", "petit_moe_router_logits",
           "petit_moe_route_hidden_workspace_bytes", "petit_moe_route_hidden")
SHAPES = [(8, 32), (32, 2880), (128, 2048), (256, 7168), (384, 7168), (1024, 16384)]
L = _lib.lib
PTR = C.c_void_p(0x1000)   # a non-null, 16-byte aligned pointer for calls that are refused before anything reads it


def test_symbols_exist():
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS


def _logits(a_type=BF16, T=4, E=8, K=64, logits=PTR, hidden=PTR, weight=PTR, ws=PTR):
    return L.petit_moe_router_logits(logits, hidden, weight, None, a_type, T, E, K, ws, None)


def _route(a_type=BF16, T=4, E=8, K=64, topk=2, desc=None, slots=None, hidden=PTR, weight=PTR, ids=PTR, w=PTR, offsets=PTR, sp=PTR, ti=PTR, ws=PTR):
    return L.petit_moe_route_hidden(hidden, weight, None, a_type, T, E, K, topk, desc, slots, ids, w, None, offsets, sp, ti, ws, None)


@pytest.mark.parametrize("call", [_logits, _route], ids=["router_logits", "route_hidden"])
def test_shape_and_dtype_refusals(call):
    assert call(K=48) == SHAPE                      # K % 32 != 0
    assert call(K=0) == SHAPE and call(K=16) == SHAPE and call(K=16384 + 32) == SHAPE
    assert call(E=0) == SHAPE and call(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == SHAPE
    assert call(T=1 << 20) == SHAPE
    for a_type in (_lib.CXX_DTYPE_FP4_E2M1, _lib.PETIT_DTYPE_FP32, 0, 77):
        assert call(a_type=a_type) == BAD
    assert call(hidden=None) == SHAPE and call(weight=None) == SHAPE
    assert call(ws=None) == SHAPE                   # the byte query is not zero for T > 0
    assert call(hidden=C.c_void_p(0x1008)) == SHAPE  # not 16-byte aligned


def test_null_outputs_and_t0():
    assert _logits(logits=None) == SHAPE
    assert _logits(T=0, logits=None, hidden=None, weight=None, ws=None) == OK
    assert _route(ids=None) == SHAPE and _route(w=None) == SHAPE
    assert _route(sp=None) == SHAPE and _route(ti=None) == SHAPE            # with an align (offsets given)
    assert _route(T=0, offsets=None, hidden=None, weight=None, ids=None, w=None, sp=None, ti=None, ws=None) == OK   # route only, nothing to do


def test_route_hidden_refuses_what_the_route_refuses():
    assert _route(topk=0) == SHAPE and _route(topk=9) == SHAPE and _route(E=128, topk=65) == SHAPE
    d = _lib.RouteDesc(7, 0, 0, 0, 0.0, None)
    assert _route(desc=C.byref(d)) == BAD                                   # a scoring that does not exist
    d = _lib.RouteDesc(_lib.PETIT_ROUTE_SOFTMAX, 0, 4, 2, 0.0, None)
    assert _route(desc=C.byref(d)) == SHAPE                                 # groups with the softmax scoring
    d = _lib.RouteDesc(_lib.PETIT_ROUTE_SIGMOID, 1, 3, 1, 0.0, None)
    assert _route(desc=C.byref(d)) == SHAPE                                 # E % n_group != 0
    s = _lib.RouteSlots(None, 4, 0, 0.0, None)
    assert _route(slots=C.byref(s)) == SHAPE                                # num_local_experts without a map
    s = _lib.RouteSlots(None, 0, 63, 0.0, None)
    assert _route(slots=C.byref(s)) == SHAPE                                # topk + S > PETIT_MOE_MAX_TOPK
    s = _lib.RouteSlots(None, 0, 0, 0.0, PTR)
    assert _route(slots=C.byref(s)) == SHAPE                                # a shared gate without shared experts


@pytest.mark.parametrize("a_type", [BF16, FP16])
@pytest.mark.parametrize("E,K", SHAPES)
def test_geometry_and_workspace(E, K, a_type):
    S, Lk = C.c_uint(0), C.c_uint(0)
    L.petit_moe_router_geometry(E, K, a_type, C.byref(S), C.byref(Lk))
    S, Lk = S.value, Lk.value
    assert Lk % 32 == 0 and Lk > 0
    assert S * Lk >= K > (S - 1) * Lk
    topk = min(E, 8)
    for T in (1, 16, 17, 1024, 4096):
        slabs = L.petit_moe_router_slabs(T, E, K, a_type)
        assert slabs in (S, 1)
        ws = L.petit_moe_router_workspace_bytes(T, E, K, a_type)
        assert ws == (slabs * T * E * 4 + 255) // 256 * 256               # rounded up to 256 bytes, as the header states
        for slots in (None, _lib.RouteSlots(None, 0, 1, 1.0, None)):
            ref = C.byref(slots) if slots is not None else None
            assert L.petit_moe_route_hidden_workspace_bytes(T, E, K, a_type, topk, ref) >= \
                ws + L.petit_moe_route_align_ex_workspace_bytes(T, topk, E, ref)
    # S and L do not depend on T: the slab count takes two values at most, S below the form switch and 1 above
    seen = {L.petit_moe_router_slabs(T, E, K, a_type) for T in range(1, 300)}
    assert seen <= {S, 1}
    # refused shapes need no workspace
    assert L.petit_moe_router_workspace_bytes(1, E, K + 8, a_type) == 0
    assert L.petit_moe_router_workspace_bytes(1, E, K, 3) == 0


def test_both_operator_layers_export_identical_signatures():
    import petit_kernel
    from petit_kernel import compiled, ops
    for name in ("moe_router_logits", "moe_route_hidden"):
        assert name in petit_kernel.__all__ and callable(getattr(petit_kernel, name))
        a, b = inspect.signature(getattr(ops, name)), inspect.signature(getattr(compiled, name))
        assert [(p.name, p.default, p.kind) for p in a.parameters.values()] == [(p.name, p.default, p.kind) for p in b.parameters.values()], name
    front = inspect.signature(petit_kernel.moe_route_hidden).parameters
    assert list(front)[:3] == ["hidden", "router_weight", "topk"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in front.items() if n not in ("hidden", "router_weight", "topk"))
    assert set(front) == set(inspect.signature(ops.moe_route_hidden).parameters)
    routed = inspect.signature(petit_kernel.fp4_moe_routed).parameters
    for name in ("router_weight", "router_bias"):
        assert routed[name].kind is inspect.Parameter.KEYWORD_ONLY and routed[name].default is None
    assert "forward_hidden" in dir(petit_kernel.GptOssExperts)

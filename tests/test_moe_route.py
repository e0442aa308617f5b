"""Routing from the router's logits: petit_moe_route / petit_moe_route_align (moe_route, moe_route_align), fp4_moe_routed and
GptOssExperts.forward_routed (include/petit_amd.h "Routing on the device, from the router's logits").

`select_np` / `weights_np` / `route_np` restate the definition in numpy: the SELECTION is written on a given float32 key matrix (key
descending, index ascending; NaN as -inf; a group's score np.float32(k1) + np.float32(k2)), the weights in float64.  On the GPU the
selection is checked EXACTLY, with nothing left out: the device's ids must be select_np of the device's own keys_out, for every token; for
the softmax scoring keys_out must equal the logits bit for bit (so the ids are a pure function of the input), for the sigmoid scoring
keys_out is compared with the float64 key.

The weight bound is derived, not tuned (u = 2^-24; the header carries the same derivation).  The kernel computes d = x - max (one rounding
of d: a relative u D / 2 on exp(d), D = the largest |x - max| among the terms), expf(d) (the device library's expf, 1 ulp = 2 u), a sum
of positive terms (6 additions deep over the lanes; with renormalize off each lane's <= 16 experts first: <= 21 deep; 1 u per level), one
correctly rounded divide (1 u) and one multiply by the scaling factor (1 u):
    softmax, renormalize   (2 + D/2) + (2 + D/2 + 6) + 1 + 1  = (12 + D) u
    softmax over all E     (2 + D/2) + (2 + D/2 + 21) + 1 + 1 = (27 + D) u
    sigmoid                s = 1 / (1 + expf(-x)): 2 + 1 + 1 = 4 u;  no renormalize 4 + 1 = 5 u;  renormalize 4 + (4 + 6 + 1) + 1 + 1 = 17 u
    sigmoid key            |error| <= 4 u s + u |key|
Each test computes D from its inputs and checks that the bound stays below 2^-16 = 256 u.  Measured on the MI355X (profiles/moe_route.md):
the largest error of any weight in these tests is recorded there in units of u.
"""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_moe import _make_layer
from test_moe_fused import align_np

DEV = "cuda"
U = 2.0 ** -24
ROOT = Path(__file__).resolve().parent.parent
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# --- the definition, restated in numpy -------------------------------------------------------------------------------------------------

def select_np(keys, topk, n_group=1, topk_group=1):
    """ids [T, topk] of the selection rule on a float32 key matrix: larger key first, the lower index among equal keys, NaN as -inf; with
    groups only the experts of the topk_group best groups (score: fp32 sum of the group's two largest keys, same rule) can be selected."""
    k = np.where(np.isnan(keys), -np.inf, keys).astype(np.float32)
    T, E = k.shape
    if n_group <= 1:
        return np.argsort(-k, axis=1, kind="stable")[:, :topk].astype(np.int32)       # stable: index ascending among equal keys
    G = E // n_group
    top2 = -np.sort(-k.reshape(T, n_group, G), axis=2)[:, :, :2]                       # largest first
    with np.errstate(invalid="ignore"):
        score = np.float32(top2[:, :, 0]) + np.float32(top2[:, :, 1])
    score = np.where(np.isnan(score), -np.inf, score).astype(np.float32)
    gsel = np.argsort(-score, axis=1, kind="stable")[:, :topk_group]
    keep = np.zeros((T, n_group), bool)
    np.put_along_axis(keep, gsel, True, axis=1)
    barred = ~np.repeat(keep, G, axis=1)
    idx = np.broadcast_to(np.arange(E), (T, E))
    order = np.lexsort((idx, -k, barred), axis=1)                                      # kept groups first, key descending, index ascending
    return order[:, :topk].astype(np.int32)


def keys_np(logits, scoring, bias=None):
    """float64 selection keys of float32-valued logits."""
    x = logits.astype(np.float64)
    if scoring == "softmax":
        return x
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    return s if bias is None else s + bias.astype(np.float64)[None, :]


def weights_np(logits, ids, scoring, renormalize, scale=1.0):
    """float64 weights of the given ids."""
    x = logits.astype(np.float64)
    xs = np.take_along_axis(x, ids.astype(np.int64), axis=1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if scoring == "softmax":
            m = x.max(axis=1, keepdims=True)
            e = np.exp(xs - m)
            denom = e.sum(axis=1, keepdims=True) if renormalize else np.exp(x - m).sum(axis=1, keepdims=True)
            w = e / denom
        else:
            s = 1.0 / (1.0 + np.exp(-xs))
            w = s / (s.sum(axis=1, keepdims=True) + 1e-20) if renormalize else s
    return w * scale


def route_np(logits, topk, scoring="softmax", renormalize=True, bias=None, n_group=1, topk_group=1, routed_scaling_factor=1.0):
    """The whole definition on the host: keys rounded to float32 as the definition says (softmax: the logits; sigmoid: fp32(s) + bias in
    fp32, from the float64 sigmoid), the selection on them, float64 weights."""
    if scoring == "softmax":
        keys = logits.astype(np.float32)
    else:
        s32 = keys_np(logits, "sigmoid").astype(np.float32)
        keys = s32 if bias is None else (s32 + bias.astype(np.float32)[None, :]).astype(np.float32)
    ids = select_np(keys, topk, n_group, topk_group)
    return weights_np(logits, ids, scoring, renormalize, routed_scaling_factor), ids, keys


def weight_bound_u(logits, ids, scoring, renormalize):
    """The derived relative bound of this case, in units of u = 2^-24 (module docstring)."""
    if scoring == "sigmoid":
        return 17.0 if renormalize else 5.0
    x = logits.astype(np.float64)
    terms = np.take_along_axis(x, ids.astype(np.int64), axis=1) if renormalize else x
    D = float((x.max(axis=1, keepdims=True) - terms).max())
    return (12.0 if renormalize else 27.0) + D


_MEASURED = {}


def _record(tag, err_u):
    _MEASURED[tag] = max(_MEASURED.get(tag, 0.0), float(err_u))
    path = os.environ.get("PETIT_ROUTE_REPORT")
    if path:
        with open(path, "w") as f:
            for k in sorted(_MEASURED):
                f.write(f"{k}: max weight error {_MEASURED[k]:.2f} u\n")


# --- without a GPU ----------------------------------------------------------------------------------------------------------------------

def test_route_abi_refusals_without_a_gpu():
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    shape, bad, ok = _lib.PETIT_ERROR_PROBLEM_SHAPE, _lib.PETIT_ERROR_BAD_ARGUMENT, _lib.PETIT_OK
    F32, SOFT, SIG = _lib.PETIT_DTYPE_FP32, _lib.PETIT_ROUTE_SOFTMAX, _lib.PETIT_ROUTE_SIGMOID
    assert _lib.PETIT_MOE_MAX_TOPK >= 32

    def desc(scoring=SOFT, renorm=1, n_group=0, topk_group=0, scale=0.0, bias=None):
        return _lib.RouteDesc(scoring, renorm, n_group, topk_group, scale, bias)

    def route(T=4, E=8, topk=2, d=None, dtype=F32, logits=p, ids=p, w=p, keys=None):
        return L.petit_moe_route(logits, dtype, T, E, topk, C.byref(d) if d is not None else None, ids, w, keys, None)

    def route_align(T=4, E=8, topk=2, d=None, dtype=F32, logits=p, ids=p, w=p, off=p, sp=p, ti=p, ws=p):
        return L.petit_moe_route_align(logits, dtype, T, E, topk, C.byref(d) if d is not None else None, ids, w, None, off, sp, ti, ws, None)

    for fn in (route, route_align):
        assert fn(topk=0) == shape
        assert fn(E=8, topk=9) == shape                                                  # topk > num_experts
        assert fn(E=256, topk=_lib.PETIT_MOE_MAX_TOPK + 1) == shape                      # above the supported maximum
        assert fn(E=0) == shape and fn(E=_lib.PETIT_MOE_MAX_EXPERTS + 1) == shape
        assert fn(T=1 << 27, E=64, topk=16) == shape                                     # T * topk >= 2^31
        assert fn(logits=None) == shape and fn(ids=None) == shape and fn(w=None) == shape
        assert fn(dtype=_lib.CXX_DTYPE_FP4_E2M1) == bad and fn(dtype=0) == bad           # a dtype that does not exist here
        assert fn(d=desc(scoring=2)) == bad and fn(d=desc(scoring=-1)) == bad
        assert fn(E=8, d=desc(SIG, n_group=3, topk_group=1)) == shape                    # E % n_group
        assert fn(E=8, d=desc(SIG, n_group=4, topk_group=0)) == shape                    # topk_group outside 1..n_group
        assert fn(E=8, d=desc(SIG, n_group=4, topk_group=5)) == shape
        assert fn(E=8, d=desc(SIG, n_group=1, topk_group=2)) == shape
        assert fn(E=8, topk=5, d=desc(SIG, n_group=4, topk_group=2)) == shape            # topk > topk_group * (E / n_group)
        assert fn(E=8, topk=1, d=desc(SIG, n_group=8, topk_group=2)) == shape            # groups of fewer than 2 experts
        assert fn(E=8, d=desc(SOFT, n_group=2, topk_group=1)) == shape                   # groups with the softmax scoring
        assert fn(E=8, d=desc(SOFT, bias=p)) == shape                                    # a bias with the softmax scoring
    assert route_align(off=None) == shape and route_align(sp=None) == shape and route_align(ti=None) == shape
    assert route_align(T=4096, topk=8, E=256, ws=None) == shape                          # several chunks need the workspace
    assert route_align(T=0, off=None) == shape                                           # (checked before the empty problem)
    # nothing to do: no launch, no pointer needed
    assert route(T=0, logits=None, ids=None, w=None) == ok
    assert route(T=0, d=desc(SIG, n_group=4, topk_group=2, bias=p), logits=None, ids=None, w=None) == ok
    for T, topk, E in ((1, 8, 256), (128, 8, 256), (129, 8, 256), (4096, 8, 1024), (4, 0, 8), (4, 8, 0), (1000, 32, 384)):
        assert L.petit_moe_route_align_workspace_bytes(T, topk, E) == L.petit_moe_align_workspace_bytes(T, topk, E)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("return_keys", [False, True])
def test_route_ops_meta_shapes(dt, return_keys):
    import petit_kernel  # noqa: F401
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    ops = torch.ops.petit_kernel
    T, E, topk = 6, 256, 8
    logits = torch.empty(T, E, dtype=TORCH_DT[dt], device="meta")
    bias = torch.empty(E, dtype=torch.float32, device="meta")
    w, ids, keys = ops.moe_route(logits, topk, 1, True, bias, 8, 4, 2.5, return_keys)
    assert w.shape == (T, topk) and w.dtype == torch.float32 and ids.shape == (T, topk) and ids.dtype == torch.int32
    assert w.device.type == "meta" and keys.dtype == torch.float32 and tuple(keys.shape) == ((T, E) if return_keys else (0,))
    w, ids, sp, off, ti, keys = ops.moe_route_align(logits, topk, 0, True, None, 1, 1, 1.0, return_keys)
    assert w.shape == (T, topk) and w.dtype == torch.float32 and ids.shape == (T, topk) and ids.dtype == torch.int32
    assert sp.shape == (T * topk,) and ti.shape == (T * topk,) and off.shape == (E + 1,) and sp.dtype == off.dtype == ti.dtype == torch.int32
    assert tuple(keys.shape) == ((T, E) if return_keys else (0,)) and keys.dtype == torch.float32


def test_package_names_the_routing_entries():
    import petit_kernel as pk
    for name in ("moe_route", "moe_route_align", "fp4_moe_routed"):
        assert name in pk.__all__ and callable(getattr(pk, name))
    assert callable(pk.GptOssExperts.forward_routed)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("renormalize", [True, False])
def test_route_np_equals_torch_topk_softmax_without_ties(seed, renormalize):
    """The yardstick itself: on float32 logits with no two equal values in a row torch's undefined tie order cannot matter, and route_np
    must give torch.topk(torch.softmax(...))'s ids and, within float32 rounding, its (renormalised) weights."""
    rng = np.random.default_rng(seed)
    T, E, topk = 64, int(rng.choice([8, 60, 256])), int(rng.choice([1, 2, 8]))
    logits = rng.standard_normal((T, E)).astype(np.float32)
    assert all(np.unique(r).size == E for r in logits)
    w, ids, keys = route_np(logits, topk, "softmax", renormalize)
    assert np.array_equal(keys.view(np.uint32), logits.view(np.uint32))
    tw, tid = torch.topk(torch.softmax(torch.from_numpy(logits), -1), topk, dim=-1)
    if renormalize:
        tw = tw / tw.sum(-1, keepdim=True)
    assert np.array_equal(ids, tid.numpy())
    assert np.abs(w - tw.double().numpy()).max() <= 16 * U * np.abs(w).max()


def test_select_np_tie_rule_and_groups_by_hand():
    k = np.array([[1, 3, 3, 2, 3, 0, np.nan, -np.inf]], np.float32)
    assert select_np(k, 8).tolist() == [[1, 2, 4, 3, 0, 5, 6, 7]]                       # NaN as -inf, then by index
    assert select_np(np.zeros((2, 6), np.float32), 3).tolist() == [[0, 1, 2]] * 2
    assert select_np(np.array([[-0.0, 0.0, -0.0]], np.float32), 2).tolist() == [[0, 1]]  # -0 equals +0
    # 4 groups of 2: scores 3, 9, 9, 5 -> groups 1 and 2 (the lower index among equal scores first); inside: key, then index
    k = np.array([[1, 2, 4, 5, 5, 4, 5, 0]], np.float32)
    assert select_np(k, 3, n_group=4, topk_group=2).tolist() == [[3, 4, 2]]
    assert select_np(k, 4, n_group=4, topk_group=2).tolist() == [[3, 4, 2, 5]]


# --- on the GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _f32(t):
    return t.detach().float().cpu().numpy()


def _check_case(pk, logits_dev, topk, tag, align=False, **routing):
    """One routing call against the definition: exact selection on the device's own keys, keys against the input, weights under the derived
    bound, renormalised rows summing to the scaling factor.  Returns the device tensors."""
    scoring, renorm = routing.get("scoring", "softmax"), routing.get("renormalize", True)
    n_group, topk_group = routing.get("n_group", 1), routing.get("topk_group", 1)
    scale, bias = routing.get("routed_scaling_factor", 1.0), routing.get("bias")
    if align:
        w, ids, sp, off, ti, keys = pk.moe_route_align(logits_dev, topk, return_keys=True, **routing)
    else:
        w, ids, keys = pk.moe_route(logits_dev, topk, return_keys=True, **routing)
    T, E = logits_dev.shape
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and keys.dtype == torch.float32
    assert ids.shape == (T, topk) and w.shape == (T, topk) and keys.shape == (T, E)
    logits = _f32(logits_dev)
    k, i, ww = keys.cpu().numpy(), ids.cpu().numpy(), w.cpu().numpy().astype(np.float64)
    # selection: exact, every token
    want = select_np(k, topk, n_group, topk_group)
    assert np.array_equal(i, want), f"{tag}: {np.count_nonzero((i != want).any(axis=1))} of {T} tokens select differently"
    if scoring == "softmax":
        assert np.array_equal(k.view(np.uint32), logits.view(np.uint32)), f"{tag}: keys_out is not the logits"
    else:
        ref_k = keys_np(logits, "sigmoid", None if bias is None else _f32(bias))
        s = keys_np(logits, "sigmoid")
        assert (np.abs(k - ref_k) <= (4 * s + np.abs(ref_k)) * U).all(), f"{tag}: key error {np.abs(k - ref_k).max() / U:.2f} u"
    # weights: float64 definition on the device's ids
    ref = weights_np(logits, i, scoring, renorm, scale)
    bound = weight_bound_u(logits, i, scoring, renorm)
    assert bound <= 256.0, f"{tag}: the derived bound {bound} u exceeds 2^-16"
    err = np.abs(ww - ref) / U
    worst = float((err / np.maximum(ref, 1e-300)).max())
    print(f"{tag}: max weight error {worst:.2f} u (bound {bound:.1f} u)")
    _record(f"{scoring}{'' if renorm else ' all-E' if scoring == 'softmax' else ' raw'}", worst)
    assert (err <= bound * ref).all(), f"{tag}: weight error {worst:.2f} u > {bound:.1f} u"
    if renorm:
        assert (np.abs(ww.sum(axis=1) - scale) <= bound * U * scale).all(), tag
    if align:
        rsp, roff, rti = align_np(i, E)
        assert np.array_equal(sp.cpu().numpy(), rsp) and np.array_equal(off.cpu().numpy(), roff) and np.array_equal(ti.cpu().numpy(), rti), tag
    return w, ids, keys


E_SET, TOPK_SET, T_SET = (8, 60, 128, 256, 384, 1024), (1, 2, 4, 8, 10, 32), (1, 7, 128, 129, 1000, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("E", E_SET)
def test_selection_exact_and_weights_softmax(pk, E, dt):
    """Every (T, topk) of the issue's sets at this E and dtype, both launch forms (moe_route, and moe_route_align which is one launch up to
    1024 entries), renormalize on and off in turn."""
    g = torch.Generator(device=DEV).manual_seed(1000 * E + len(dt))
    n = 0
    for T in T_SET:
        logits = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
        for topk in TOPK_SET:
            if topk > E:
                with pytest.raises(RuntimeError):
                    pk.moe_route(logits, topk)
                continue
            n += 1
            _check_case(pk, logits, topk, f"softmax E {E} topk {topk} T {T} {dt}", align=bool(n & 1), scoring="softmax", renormalize=bool(n & 2))


@pytest.mark.gpu
@pytest.mark.parametrize("E", E_SET)
def test_selection_exact_and_weights_sigmoid(pk, E):
    """The same sets on the sigmoid scoring without groups (a bias in every other case), the dtype taking turns."""
    g = torch.Generator(device=DEV).manual_seed(77 + E)
    bias = torch.randn(E, device=DEV, generator=g) * 0.1
    n = 0
    for T in T_SET:
        for topk in TOPK_SET:
            if topk > E:
                continue
            n += 1
            dt = ("f32", "bf16", "f16")[n % 3]
            logits = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
            _check_case(pk, logits, topk, f"sigmoid E {E} topk {topk} T {T} {dt}", align=bool(n & 1), scoring="sigmoid", renormalize=bool(n & 2),
                        bias=bias if n & 4 else None, routed_scaling_factor=2.5 if n & 8 else 1.0)


GROUPED = {
    "deepseek-v3": dict(E=256, topk=8, n_group=8, topk_group=4, routed_scaling_factor=2.5, bias=True),
    "kimi-one-group": dict(E=384, topk=8, n_group=1, topk_group=1, routed_scaling_factor=2.827, bias=True),
    "groups-of-two": dict(E=128, topk=8, n_group=64, topk_group=6, routed_scaling_factor=1.0, bias=True),
    "groups-of-two-wide": dict(E=1024, topk=32, n_group=512, topk_group=20, routed_scaling_factor=1.0, bias=False),
    "groups-of-128": dict(E=1024, topk=10, n_group=8, topk_group=3, routed_scaling_factor=1.0, bias=True),
    "groups-of-12": dict(E=60, topk=4, n_group=5, topk_group=2, routed_scaling_factor=1.0, bias=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", sorted(GROUPED))
def test_selection_exact_grouped(pk, name, dt):
    c = dict(GROUPED[name])
    E, topk = c.pop("E"), c.pop("topk")
    g = torch.Generator(device=DEV).manual_seed(len(name) + len(dt))
    bias = torch.randn(E, device=DEV, generator=g) * 0.1 if c.pop("bias") else None
    for n, T in enumerate(T_SET if E < 1024 or c["n_group"] < 512 else (1, 7, 129)):
        logits = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
        _check_case(pk, logits, topk, f"{name} T {T} {dt}", align=bool(n & 1), scoring="sigmoid", renormalize=True, bias=bias, **c)


@pytest.mark.gpu
def test_ties_on_purpose(pk):
    g = torch.Generator(device=DEV).manual_seed(5)
    # bf16 standard-normal logits: the k-th and (k+1)-th largest are equal in several percent of the tokens
    for E, topk in ((8, 2), (128, 8), (256, 8), (1024, 8)):
        logits = torch.randn(4096, E, device=DEV, generator=g).bfloat16()
        srt = np.sort(_f32(logits), axis=1)[:, ::-1]
        tied = float((srt[:, topk - 1] == srt[:, topk]).mean())
        print(f"E {E} top-{topk}: boundary ties in {100 * tied:.1f} % of the tokens")
        assert tied > 0 or E == 8
        _check_case(pk, logits, topk, f"bf16 ties E {E}", scoring="softmax")
        _check_case(pk, logits, topk, f"bf16 ties sigmoid E {E}", align=True, scoring="sigmoid")
    # four distinct values
    vals = torch.tensor([-1.5, 0.0, 0.25, 3.0], device=DEV)
    for E, topk, dt in ((60, 10, "f32"), (256, 8, "bf16"), (1024, 32, "f16")):
        logits = vals[torch.randint(0, 4, (1000, E), device=DEV, generator=g)].to(TORCH_DT[dt])
        _check_case(pk, logits, topk, f"four values E {E}", scoring="softmax", renormalize=False)
        _check_case(pk, logits, topk, f"four values sigmoid E {E}", scoring="sigmoid")
    _check_case(pk, vals[torch.randint(0, 4, (129, 256), device=DEV, generator=g)], 8, "four values, DeepSeek groups", align=True, scoring="sigmoid",
                n_group=8, topk_group=4)
    # all logits equal: ids 0 .. topk-1; with groups the first topk_group groups
    for E, topk in ((8, 8), (256, 8), (1024, 32)):
        for value in (0.0, -0.0, 1.25):
            logits = torch.full((7, E), value, device=DEV)
            for scoring in ("softmax", "sigmoid"):
                w, ids, _ = _check_case(pk, logits, topk, f"all equal E {E}", scoring=scoring)
                assert (ids.cpu() == torch.arange(topk, dtype=torch.int32)).all()
                assert (w == w[:, :1]).all()
    w, ids, _ = _check_case(pk, torch.zeros(5, 256, device=DEV), 8, "all equal, groups", scoring="sigmoid", n_group=8, topk_group=4)
    assert (ids.cpu() == torch.arange(8, dtype=torch.int32)).all()
    w, ids, _ = _check_case(pk, torch.zeros(5, 64, device=DEV), 12, "all equal, small groups", scoring="sigmoid", n_group=16, topk_group=4)
    assert (ids.cpu() == torch.arange(12, dtype=torch.int32)).all()                    # groups 0..2 fully, then group 3


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_special_values(pk, scoring, dt):
    """Rows holding -inf, +inf and NaN: ids as the rule says on keys_out, distinct and in range; the finite rows of the same batch are
    bit for bit what they are when routed alone, weights included."""
    E, topk, T = 256, 8, 300
    g = torch.Generator(device=DEV).manual_seed(3)
    clean = torch.randn(T, E, device=DEV, generator=g).to(TORCH_DT[dt])
    logits = clean.clone()
    rng = np.random.default_rng(4)
    special = np.zeros(T, bool)
    for t in range(0, T, 3):
        special[t] = True
        cols = torch.from_numpy(rng.choice(E, int(rng.integers(1, E // 2)), replace=False)).to(DEV)
        kind = (t // 3) % 5
        logits[t, cols] = (float("nan"), float("-inf"), float("inf"))[kind] if kind < 3 else float("nan")
        if kind == 3:
            logits[t] = float("nan")                                                   # a whole row of NaN
        if kind == 4:
            logits[t, cols[: len(cols) // 2]] = float("-inf")                          # NaN and -inf in one row
    kw = dict(scoring=scoring, renormalize=True)
    w, ids, keys = pk.moe_route(logits, topk, return_keys=True, **kw)
    w2, ids2, sp, off, ti, keys2 = pk.moe_route_align(logits[:100].contiguous(), topk, return_keys=True, **kw)
    i = ids.cpu().numpy()
    assert np.array_equal(i, select_np(keys.cpu().numpy(), topk))
    assert ((i >= 0) & (i < E)).all() and all(np.unique(r).size == topk for r in i)
    assert torch.equal(ids[:100], ids2) and torch.equal(keys[:100].view(torch.int32), keys2.view(torch.int32))
    if scoring == "softmax":
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), _f32(logits).view(np.uint32))
    fin = torch.from_numpy(~special).to(DEV)
    wc, idc = pk.moe_route(clean, topk, **kw)
    assert torch.equal(ids[fin], idc[fin]) and torch.equal(w[fin].view(torch.int32), wc[fin].view(torch.int32))
    assert torch.equal(w[:100][fin[:100]].view(torch.int32), w2[fin[:100]].view(torch.int32))
    # -inf alone does not make a row special for the softmax weights: exp(-inf) = 0
    if scoring == "softmax":
        part = clean[:64].clone()
        part[:, ::2] = float("-inf")
        w3, ids3 = pk.moe_route(part, topk, **kw)
        ref = weights_np(_f32(part), ids3.cpu().numpy(), "softmax", True)
        x = _f32(part)
        D = float((x.max(axis=1, keepdims=True) - np.take_along_axis(x, ids3.cpu().numpy().astype(np.int64), axis=1)).max())
        assert (np.abs(w3.cpu().numpy() - ref) <= (12 + D) * U * ref).all()


@pytest.mark.gpu
def test_route_align_is_route_then_align_and_bindings_agree(pk):
    """moe_route_align's five outputs (and the keys) equal moe_route followed by moe_align_device, bit for bit, on both sides of 1024 entries;
    moe_align_device still equals align_np; the ctypes layer and the compiled ops return the same tensors; repeated launches repeat."""
    from petit_kernel import compiled, ops
    assert compiled.available()
    g = torch.Generator(device=DEV).manual_seed(9)
    cases = [(1, 8, 256), (128, 8, 256), (129, 8, 256), (1024, 1, 60), (1025, 1, 60), (32, 32, 384), (33, 32, 384), (4096, 8, 1024), (102, 10, 128),
             (103, 10, 128), (0, 8, 256)]
    for n, (T, topk, E) in enumerate(cases):
        logits = torch.randn(T, E, device=DEV, generator=g).to((torch.float32, torch.bfloat16, torch.float16)[n % 3])
        routing = [dict(scoring="softmax", renormalize=True), dict(scoring="sigmoid", renormalize=True, routed_scaling_factor=2.5,
                                                                    bias=torch.randn(E, device=DEV, generator=g) * 0.1),
                   dict(scoring="softmax", renormalize=False)][n % 3]
        if E == 256 and routing["scoring"] == "sigmoid":
            routing.update(n_group=8, topk_group=4)
        w, ids, keys = pk.moe_route(logits, topk, return_keys=True, **routing)
        sp, off, ti = pk.moe_align_device(ids, E)
        rsp, roff, rti = align_np(ids.cpu().numpy().reshape(T, topk), E)
        assert np.array_equal(sp.cpu().numpy(), rsp) and np.array_equal(off.cpu().numpy(), roff) and np.array_equal(ti.cpu().numpy(), rti)
        for layer in (pk, compiled, ops):
            for _ in range(2):
                fw, fids, fsp, foff, fti, fkeys = layer.moe_route_align(logits, topk, return_keys=True, **routing)
                assert torch.equal(fids, ids) and torch.equal(fw.view(torch.int32), w.view(torch.int32)), (T, topk, E)
                assert torch.equal(fsp, sp) and torch.equal(foff, off) and torch.equal(fti, ti), (T, topk, E)
                assert torch.equal(fkeys.view(torch.int32), keys.view(torch.int32))
            lw, lids = layer.moe_route(logits, topk, **routing)
            assert torch.equal(lids, ids) and torch.equal(lw.view(torch.int32), w.view(torch.int32))
            assert len(layer.moe_route_align(logits, topk, **routing)) == 5
        if T == 0:
            assert (off == 0).all() and off.numel() == E + 1


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["nvfp4", "mxfp4"])
def test_routed_layer_is_the_layer(pk, kind, dt):
    """fp4_moe_routed equals fp4_moe_fused / fp4_moe_native on moe_route's outputs bit for bit: plain, and with biases and swiglu_oai;
    several routings; T * topk on both sides of 1024."""
    from test_moe_native import _native_layer
    E, hid, inter = 8, 1024, 512
    w13, w2, b13, s13, b2, s2 = _native_layer(pk, kind[:2], E, hid, inter, 23)
    g = torch.Generator(device=DEV).manual_seed(2)
    bias13 = (torch.randn(E, 2 * inter, device=DEV, generator=g) * 0.5).to(dt)
    bias2 = (torch.randn(E, hid, device=DEV, generator=g) * 0.5).to(dt)
    routings = [dict(scoring="softmax", renormalize=True), dict(scoring="softmax", renormalize=False),
                dict(scoring="sigmoid", renormalize=True, n_group=4, topk_group=2, routed_scaling_factor=2.5,
                     bias=torch.randn(E, device=DEV, generator=g) * 0.1)]
    for n, (T, topk) in enumerate(((1, 2), (16, 4), (300, 2), (600, 2))):
        x = torch.randn(T, hid, device=DEV, generator=g).to(dt)
        logits = torch.randn(T, E, device=DEV, generator=g).to((torch.float32, torch.bfloat16, torch.float16)[n % 3])
        for routing in routings:
            tw, ids = pk.moe_route(logits, topk, **routing)
            for extra in (dict(), dict(bias13=bias13, bias2=bias2, activation="swiglu_oai")):
                fused = pk.fp4_moe_fused(x, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, tw, ids, kind, **extra)
                got = pk.fp4_moe_routed(x, logits, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, topk, kind, path="fused", **extra, **routing)
                assert got.dtype == dt and torch.equal(_bits(got), _bits(fused)), (T, topk, routing["scoring"], bool(extra))
                native = pk.fp4_moe_native(x, b13, s13, w13.gsd, b2, s2, w2.gsd, tw, ids, kind=kind, activations="mxfp8", **extra)
                got = pk.fp4_moe_routed(x, logits, b13, s13, w13.gsd, b2, s2, w2.gsd, topk, kind, path="native", activations="mxfp8", **extra,
                                        **routing)
                assert torch.equal(_bits(got), _bits(native)), (T, topk, routing["scoring"], bool(extra), "native")
    with pytest.raises(RuntimeError):
        pk.fp4_moe_routed(x, logits[:, :4].contiguous(), w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, 2, kind)
    with pytest.raises(RuntimeError):
        pk.fp4_moe_routed(x, logits, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, 2, kind, path="other")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "native"])
def test_gptoss_forward_routed_is_forward(pk, path):
    from test_gptoss import _input, synth_checkpoint
    ck = synth_checkpoint(8, 352, 352, 31)
    ex = pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in ck.items()})
    g = torch.Generator(device=DEV).manual_seed(6)
    for T in (1, 5, 300):
        x = _input(T, 352, T).to(DEV)
        logits = torch.randn(T, 8, device=DEV, generator=g).bfloat16()
        tw, ids = pk.moe_route(logits, 4, scoring="softmax", renormalize=True)
        # gpt-oss's router: the top-k logits, then softmax over the k
        top = torch.topk(logits.float(), 4, dim=-1)
        assert (tw - torch.softmax(top.values, -1)).abs().max() <= 1e-6
        want = ex.forward(x, tw, ids, path=path)
        got = ex.forward_routed(x, logits, topk=4, path=path)
        assert got.shape == (T, 352) and torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_routed_layer_graph_replay_with_changing_logits(pk):
    """fp4_moe_routed captured once under torch.cuda.graph on one stream (no parallel branches), replayed with three different logit
    tensors copied into the captured input: each replay equals the eager call, and repeated launches are bit-identical."""
    E, topk, hid, inter, T = 8, 2, 1024, 512, 16
    w13, w2 = _make_layer(pk, "nv", E, hid, inter, 77)
    x = torch.randn(T, hid, device=DEV).to(torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(8)
    bias = torch.randn(E, device=DEV, generator=g) * 0.1
    kw = dict(scoring="sigmoid", renormalize=True, bias=bias, n_group=4, topk_group=2, routed_scaling_factor=2.5)

    def layer(xx, ll):
        return pk.fp4_moe_routed(xx, ll, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, topk, "nvfp4", **kw)

    sx, sl = x.clone(), torch.randn(T, E, device=DEV, generator=g).bfloat16()
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
        xi = torch.randn(T, hid, device=DEV, generator=g).to(torch.bfloat16)
        li = torch.randn(T, E, device=DEV, generator=g).bfloat16() if i < 2 else torch.zeros(T, E, device=DEV).bfloat16()
        sx.copy_(xi)
        sl.copy_(li)
        graph.replay()
        torch.cuda.synchronize()
        eager, again = layer(xi, li), layer(xi, li)
        torch.cuda.synchronize()
        assert torch.equal(_bits(eager), _bits(again))
        assert torch.equal(_bits(out), _bits(eager)), f"replay {i} differs from the eager call"


_TRACE_CHILD = """
import sys
import torch
sys.path[:0] = [{root!r}, {root!r} + "/petit-kernel_amd", {root!r} + "/tests"]
import petit_kernel as pk
from test_moe import _make_layer
T, topk, calls = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
E, hid, inter = 8, 1024, 512
w13, w2 = _make_layer(pk, "nv", E, hid, inter, 5)
x = torch.randn(T, hid, device="cuda").bfloat16()
logits = torch.randn(T, E, device="cuda")
torch.cuda.synchronize()
for _ in range(calls):
    out = pk.fp4_moe_routed(x, logits, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, topk, "nvfp4", scoring="softmax", renormalize=True)
torch.cuda.synchronize()
"""


def _traced_kernel_count(tmp_path, T, topk, calls):
    import csv
    import shutil
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    script = tmp_path / "child.py"
    script.write_text(_TRACE_CHILD.format(root=str(ROOT)))
    out = tmp_path / f"trace_{T}_{topk}_{calls}"
    cmd = ["timeout", "-k", "10", "240", rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "-o", "run", "--",
           sys.executable, str(script), str(T), str(topk), str(calls)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = list(out.rglob("*kernel_trace.csv"))
    assert len(files) == 1, files
    with open(files[0]) as f:
        names = [row["Kernel_Name"] for row in csv.DictReader(f)]
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("T,topk,launches", [(512, 2, 4), (513, 2, 7)])
def test_launch_count_under_kernel_trace(pk, tmp_path, T, topk, launches):
    """A condition, not a measurement: under rocprofv3 --kernel-trace --stats one fp4_moe_routed(path="fused") call is exactly 4 kernel launches
    at T * topk <= 1024 and 7 above.  Counted as (kernels of a process that makes three calls - kernels of one that makes one) / 2, so the
    set-up launches cancel."""
    one = _traced_kernel_count(tmp_path, T, topk, 1)
    three = _traced_kernel_count(tmp_path, T, topk, 3)
    assert len(three) - len(one) == 2 * launches, (len(one), len(three))
    ours = [n for n in three if "moe_route" in n]
    assert len(ours) == 3, ours                                                          # one route (+ align) launch per call
    report = os.environ.get("PETIT_ROUTE_TRACE_REPORT")
    if report:
        tail = three[len(three) - launches:]
        with open(report, "a") as f:
            short = [re.split(r"[<(]", n.replace("void ", "").replace("(anonymous namespace)::", "").replace("petit_amd::", ""))[0] for n in tail]
            f.write(f"T {T} topk {topk}: {launches} launches per call: " + ", ".join(short) + "\n")

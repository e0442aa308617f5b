"""The router's GEMM on the GPU (include/petit_amd.h "The router's GEMM"): moe_router_logits, moe_route_hidden, fp4_moe_routed(router_weight=...)
and GptOssExperts.forward_hidden.

Shapes are the smallest that reach every path: E in {8, 24, 128, 257} (not a multiple of 16, a ragged last n-tile, several n-blocks), K in
{32, L, L + 32, 2880} with L the slice length of that E (one k-step, exactly one slice, a ragged second slice, a model's K), T in
{1, 7, 16, 17, 65} and one T on each side of the form switch, found through petit_moe_router_slabs; bfloat16 and float16.

The accuracy bound is derived, not tuned (u = 2^-24): a product of two bf16 or two fp16 values is exact in fp32, and each of the at most
K + S + 1 accumulation steps (K products joining a slice's sum, S slice sums, the bias) errs by at most one ulp -- 2 u relative, rounding or
truncation alike -- of a magnitude no larger than sum_k |a_k w_k| + |bias|:
    |logit - exact| <= 2 u (K + S + 1) (sum_k |a_k w_k| + |bias|)
The largest error measured on the MI355X is recorded in profiles/moe_router.md in units of u sum_k |a_k w_k| (2.02 bf16, 2.29 fp16).
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_moe import _make_layer

DEV = "cuda"
U = 2.0 ** -24
ROOT = Path(__file__).resolve().parent.parent
E_SET = (8, 24, 128, 257)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


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


def _k_set(E):
    from petit_kernel import ops
    L = ops.router_geometry(E, 32)[1]
    assert ops.router_geometry(E, L) == (1, L) and ops.router_geometry(E, L + 32) == (2, L)   # exactly one slice; a ragged second one
    assert ops.router_geometry(E, 2880)[0] > 2
    return (32, L, L + 32, 2880)


def _switch(E, K, dtype=torch.bfloat16):
    """(largest T of the split form, smallest T of the whole form) for a K of several slices."""
    from petit_kernel import ops
    S = ops.router_geometry(E, K, dtype)[0]
    assert S > 1 and ops.router_slabs(1, E, K, dtype) == S
    T = 1
    while ops.router_slabs(T + 1, E, K, dtype) == S:
        T += 1
        assert T < 1 << 16
    assert ops.router_slabs(T + 1, E, K, dtype) == 1
    return T, T + 1


def _t_set(E):
    return sorted({1, 7, 16, 17, 65, *_switch(E, 2880)})


def _exact_inputs(T, E, K, dtype, seed):
    """Small integers with many zeros and sign flips: every partial sum is an integer below 2^24, exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (T, K), generator=g) * (torch.rand(T, K, generator=g) < 0.5)
    w = torch.randint(-8, 9, (E, K), generator=g) * (torch.rand(E, K, generator=g) < 0.5)
    b = torch.randint(-3, 4, (E,), generator=g)
    ref = (a.double() @ w.double().T).long() + b                                            # integers below 2^24: exact in float64, as int64
    assert int((a.abs().double() @ w.abs().double().T).max()) + 3 < 1 << 24
    return a.to(dtype).to(DEV), w.to(dtype).to(DEV), b.float().to(DEV), ref


def _random_inputs(T, E, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(T, K, generator=g).to(dtype)
    w = (torch.randn(E, K, generator=g) / K ** 0.5).to(dtype)
    b = torch.randn(E, generator=g)
    return a.to(DEV), w.to(DEV), b.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# --- 1. exact ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("E", E_SET)
def test_exact_on_small_integers(pk, E, dt):
    """moe_router_logits equals the int64 matmul exactly: every (K, T) of the module's sets, both forms, both operator layers, with and
    without the bias."""
    dtype = DTYPES[dt]
    ts = _t_set(E)
    for K in _k_set(E):
        a, w, b, ref = _exact_inputs(max(ts), E, K, dtype, 1000 * E + K)
        for T in ts:
            for name, layer in _layers().items():
                for bias in (b, None):
                    out = layer.moe_router_logits(a[:T].contiguous(), w, bias)
                    want = (ref[:T] if bias is not None else ref[:T] - b.cpu().long()).to(torch.float32)
                    assert out.dtype == torch.float32 and out.shape == (T, E)
                    assert torch.equal(out.cpu(), want), (name, E, K, T, dt, bias is not None)


# --- 2. the bound on random inputs -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("E", E_SET)
def test_error_bound_on_random_inputs(pk, E, dt):
    """|logit - f64| <= 2 u (K + S + 1) (sum |a w| + |bias|) for every element of every (K, T); prints the largest error in u sum |a w|."""
    from petit_kernel import ops
    dtype = DTYPES[dt]
    ts = _t_set(E)
    worst = 0.0
    for K in _k_set(E):
        S = ops.router_geometry(E, K, dtype)[0]
        a, w, b = _random_inputs(max(ts), E, K, dtype, 7 * E + K)
        a64, w64, b64 = a.cpu().double(), w.cpu().double(), b.cpu().double()
        ref = a64 @ w64.T + b64
        mag = a64.abs() @ w64.abs().T
        for T in ts:
            out = pk.moe_router_logits(a[:T].contiguous(), w, b).cpu().double()
            err = (out - ref[:T]).abs()
            bound = 2 * U * (K + S + 1) * (mag[:T] + b64.abs())
            worst = max(worst, float((err / (U * mag[:T])).max()))
            assert bool((err <= bound).all()), (E, K, T, dt, float((err / bound).max()))
    print(f"router error E {E} {dt}: max |err| = {worst:.3f} u sum|a w|")


# --- 3. composition ----------------------------------------------------------------------------------------------------------------------

def _routings(E, T):
    """(name, topk, routing keywords) of the routings the composition test runs at E experts."""
    g = torch.Generator().manual_seed(E)
    topk = min(E, 8) if E != 8 else 2
    out = [("softmax", topk, dict(scoring="softmax", renormalize=True)),
           ("softmax-all", topk, dict(scoring="softmax", renormalize=False)),
           ("sigmoid", topk, dict(scoring="sigmoid", renormalize=True))]
    if E % 8 == 0 and E >= 24:
        sb = (torch.randn(E, generator=g) * 0.1).to(DEV)
        out.append(("deepseek", topk, dict(scoring="sigmoid", renormalize=True, bias=sb, n_group=8 if E >= 64 else 4,
                                           topk_group=4 if E >= 64 else 3, routed_scaling_factor=2.5)))
    emap = torch.full((E,), -1, dtype=torch.int32)
    emap[E // 2:] = torch.arange(E - E // 2, dtype=torch.int32)
    out.append(("expert-map", topk, dict(scoring="softmax", renormalize=True, expert_map=emap.to(DEV), num_local_experts=E - E // 2)))
    gate = torch.randn(T, 1, generator=g).to(DEV)
    out.append(("shared", topk, dict(scoring="sigmoid", renormalize=True, num_shared=1, shared_weight=0.5, shared_gate_logits=gate)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("inputs", ["exact", "random"])
@pytest.mark.parametrize("E", (8, 24, 128, 257, 600))
def test_route_hidden_is_route_on_the_logits(pk, E, inputs):
    """moe_route_hidden(...) equals moe_route_align / moe_route on moe_router_logits(...) in every output, bit for bit: each routing, both
    forms of the GEMM, one chunk and several, with and without the router bias; the softmax keys are the logits.  E = 600: the finishing
    launch in front of the 16-key route kernel.  The exact inputs are tie-rich: ties go to the lower index in both."""
    dtype = torch.bfloat16 if E != 24 else torch.float16
    L = _k_set(E)[1]
    split_t, whole_t = _switch(E, 2880)
    for K in (L + 32, 2880) if E != 600 else (L + 32,):
        for T in (7, split_t, whole_t, 200):
            if inputs == "exact":
                a, w, b, _ = _exact_inputs(T, E, K, dtype, E + K + T)
            else:
                a, w, b = _random_inputs(T, E, K, dtype, E + K + T)
            for name, topk, kw in _routings(E, T):
                for rb in (b, None):
                    logits = pk.moe_router_logits(a, w, rb)
                    for align in (True, False):
                        got = pk.moe_route_hidden(a, w, topk, router_bias=rb, align=align, return_keys=True, **kw)
                        want = (pk.moe_route_align if align else pk.moe_route)(logits, topk, return_keys=True, **kw)
                        assert len(got) == len(want) == (6 if align else 3)
                        for i, (x, y) in enumerate(zip(got, want)):
                            assert _same(x, y), (name, E, K, T, align, rb is not None, i)
                        if kw["scoring"] == "softmax":
                            assert _same(got[-1], logits), (name, E, K, T)


# --- 4. batch invariance -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("E", (24, 128))
def test_a_rows_logits_do_not_depend_on_its_batch(pk, E, dt):
    """Row r of moe_router_logits(batch) equals moe_router_logits(batch[r : r + 1]) bit for bit, for a batch of 65 rows and for one on the
    whole-form side of the switch (the single row always runs the split form), and the same row among other rows, at another position,
    gives the same bits."""
    dtype, K = DTYPES[dt], 2880
    whole_t = _switch(E, K, dtype)[1]
    for T in sorted({65, whole_t + 130}):
        a, w, b = _random_inputs(T, E, K, dtype, T + E)
        full = pk.moe_router_logits(a, w, b)
        other, _, _ = _random_inputs(T + 9, E, K, dtype, T + E + 1)
        for r in (0, 15, 16, T - 1):
            alone = pk.moe_router_logits(a[r:r + 1].contiguous(), w, b)
            assert _same(alone[0], full[r]), (E, T, r)
            pos = (r + 5) % (T + 9)
            other[pos] = a[r]
            assert _same(pk.moe_router_logits(other, w, b)[pos], full[r]), (E, T, r, pos)


# --- 5. the write contract, through the C ABI --------------------------------------------------------------------------------------------

class _Guarded:
    """A caller buffer of `count` 4-byte elements between two guard zones, everything poisoned."""
    GUARD = 1024
    POISON = 0x7FC5A5A5  # (a NaN as float32)

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
            assert bool((self.inside() != self.POISON).all()), f"{what}: an element was not written"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTYPES))
def test_write_contract_through_the_c_abi(pk, dt):
    """T = 17, E = 24, K = L + 32 on poisoned, guarded buffers: every logit, id, weight, key, offset and index is written, nothing lands
    outside them, and nothing past the bytes the workspace queries declare."""
    from petit_kernel import _lib, ops
    dtype = DTYPES[dt]
    a_type = ops._a_type(dtype)
    T, E, topk = 17, 24, 4
    K = _k_set(E)[2]
    a, w, b = _random_inputs(T, E, K, dtype, 5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    ws_bytes = int(_lib.lib.petit_moe_router_workspace_bytes(T, E, K, a_type))
    assert ws_bytes % 4 == 0 and ws_bytes > 0
    logits, ws = _Guarded(T * E), _Guarded(ws_bytes // 4)
    rc = _lib.lib.petit_moe_router_logits(logits.ptr, ptr(a), ptr(w), ptr(b), a_type, T, E, K, ws.ptr, stream)
    torch.cuda.synchronize()
    assert rc == _lib.PETIT_OK
    logits.check("logits")
    ws.check("router workspace", all_written=False)
    assert _same(logits.inside().view(torch.float32).reshape(T, E), pk.moe_router_logits(a, w, b))

    slots = _lib.RouteSlots(None, 0, 1, 1.0, None)
    desc = _lib.RouteDesc(_lib.PETIT_ROUTE_SOFTMAX, 1, 0, 0, 0.0, None)
    ws_bytes = int(_lib.lib.petit_moe_route_hidden_workspace_bytes(T, E, K, a_type, topk, C.byref(slots)))
    n_slots = topk + 1
    ids, wts, keys = _Guarded(T * n_slots), _Guarded(T * n_slots), _Guarded(T * E)
    offsets, sp, ti, ws = _Guarded(E + 1 + 1), _Guarded(T * n_slots), _Guarded(T * n_slots), _Guarded(ws_bytes // 4)
    rc = _lib.lib.petit_moe_route_hidden(ptr(a), ptr(w), ptr(b), a_type, T, E, K, topk, C.byref(desc), C.byref(slots), ids.ptr, wts.ptr, keys.ptr,
                                         offsets.ptr, sp.ptr, ti.ptr, ws.ptr, stream)
    torch.cuda.synchronize()
    assert rc == _lib.PETIT_OK
    for name, buf in (("topk_ids", ids), ("topk_weights", wts), ("keys_out", keys), ("expert_offsets", offsets), ("sorted_pos", sp),
                      ("token_index", ti)):
        buf.check(name)
    ws.check("route_hidden workspace", all_written=False)
    want = pk.moe_route_hidden(a, w, topk, router_bias=b, return_keys=True, num_shared=1)
    got = (wts.inside().view(torch.float32).reshape(T, n_slots), ids.inside().reshape(T, n_slots), sp.inside(), offsets.inside(), ti.inside(),
           keys.inside().view(torch.float32).reshape(T, E))
    for i, (x, y) in enumerate(zip(got, want)):
        assert _same(x, y), i


# --- 6. the layers -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "native"])
def test_layer_from_the_hidden_state(pk, path):
    """fp4_moe_routed(hidden, None, ..., router_weight=W, router_bias=b) equals fp4_moe_routed(hidden, moe_router_logits(hidden, W, b), ...)
    bit for bit: T = 7, E = 8, hidden 1024."""
    E, topk, hid, inter, T = 8, 2, 1024, 512, 7
    w13, w2 = _make_layer(pk, "nv", E, hid, inter, 91)
    x, W, b = _random_inputs(T, E, hid, torch.bfloat16, 3)
    args = (w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, topk, "nvfp4")
    kw = dict(path=path, scoring="softmax", renormalize=True, transient=path == "native")   # (native on the packed tensors: no resident images)
    got = pk.fp4_moe_routed(x, None, *args, router_weight=W, router_bias=b, **kw)
    want = pk.fp4_moe_routed(x, pk.moe_router_logits(x, W, b), *args, **kw)
    torch.cuda.synchronize()
    assert got.shape == (T, hid) and torch.equal(got.view(torch.int16), want.view(torch.int16))
    with pytest.raises(RuntimeError, match="router_logits must be None"):
        pk.fp4_moe_routed(x, pk.moe_router_logits(x, W, b), *args, router_weight=W, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "native"])
def test_gptoss_forward_hidden(pk, path):
    """GptOssExperts.forward_hidden equals forward_routed on moe_router_logits of the unpadded x, at test_gptoss.py's small size
    (E = 8, H = I = 352 -> 512, top-4)."""
    from test_gptoss import _input, synth_checkpoint
    T, E, H = 5, 8, 352
    ck = synth_checkpoint(E, H, H, 33)
    ex = pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in ck.items()})
    x = _input(T, H, 9).to(DEV)
    _, W, b = _random_inputs(1, E, H, torch.bfloat16, 4)
    got = ex.forward_hidden(x, W, b, topk=4, path=path)
    want = ex.forward_routed(x, pk.moe_router_logits(x, W, b), topk=4, path=path)
    torch.cuda.synchronize()
    assert got.shape == (T, H) and torch.equal(got.view(torch.int16), want.view(torch.int16))


# --- 7. refusals -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("layer", ["ctypes", "compiled"])
def test_python_refusals(pk, layer):
    impl = _layers()[layer]
    a, w, b = _random_inputs(4, 8, 64, torch.bfloat16, 1)
    wide = torch.randn(4, 128, device=DEV).bfloat16()
    for call in (lambda h, ww, bb: impl.moe_router_logits(h, ww, bb), lambda h, ww, bb: impl.moe_route_hidden(h, ww, 2, bb)):
        with pytest.raises(RuntimeError, match="hidden must be contiguous"):
            call(wide[:, ::2], w, b)
        with pytest.raises(RuntimeError, match="router_weight must be contiguous"):
            call(a, torch.randn(8, 128, device=DEV).bfloat16()[:, ::2], b)
        with pytest.raises(RuntimeError, match="router_bias must be contiguous"):
            call(a, w, torch.randn(16, device=DEV)[::2])
        with pytest.raises(RuntimeError, match="router_weight must have hidden's dtype"):
            call(a, w.half(), b)
        with pytest.raises(RuntimeError, match="router_bias must be float32"):
            call(a, w, b.bfloat16())
        with pytest.raises(RuntimeError, match="k must be a multiple of 32"):
            call(a[:, :48].contiguous(), w[:, :48].contiguous(), b)
        assert call(a, w, b) is not None


# --- 8. launch counts --------------------------------------------------------------------------------------------------------------------

_TRACE_CHILD = """
import sys
import torch
sys.path[:0] = [{root!r}, {root!r} + "/petit-kernel_amd", {root!r} + "/tests"]
import petit_kernel as pk
from test_moe import _make_layer
what, calls = sys.argv[1], int(sys.argv[2])
T, topk, E, hid, inter = 64, 2, 8, 1024, 512
w13, w2 = _make_layer(pk, "nv", E, hid, inter, 5)
x = torch.randn(T, hid, device="cuda").bfloat16()
W = (torch.randn(E, hid, device="cuda") / 32).bfloat16()
b = torch.randn(E, device="cuda")
torch.cuda.synchronize()
for _ in range(calls):
    if what == "layer":
        out = pk.fp4_moe_routed(x, None, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, topk, "nvfp4", path="fused", router_weight=W, router_bias=b,
                                scoring="softmax", renormalize=True)
    else:
        out = pk.moe_route_hidden(x, W, topk, router_bias=b)
torch.cuda.synchronize()
"""


def _traced_kernel_names(tmp_path, what, calls):
    import csv
    import shutil
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    script = tmp_path / "child.py"
    script.write_text(_TRACE_CHILD.format(root=str(ROOT)))
    out = tmp_path / f"trace_{what}_{calls}"
    cmd = ["timeout", "-k", "10", "240", rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "-o", "run", "--",
           sys.executable, str(script), what, str(calls)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = list(out.rglob("*kernel_trace.csv"))
    assert len(files) == 1, files
    with open(files[0]) as f:
        return [row["Kernel_Name"] for row in csv.DictReader(f)]


@pytest.mark.gpu
@pytest.mark.parametrize("what,launches", [("layer", 5), ("route", 2)])
def test_launch_count_under_kernel_trace(pk, tmp_path, what, launches):
    """A condition, not a measurement: under rocprofv3 --kernel-trace --stats one fp4_moe_routed(path="fused", router_weight=...) call at
    T * topk <= 1024 is exactly 5 kernel launches (the 4 of the layer from the logits and the router GEMM), one moe_route_hidden call 2.
    Counted as (kernels of a process that makes three calls - kernels of one that makes one) / 2, so the set-up launches cancel."""
    one = _traced_kernel_names(tmp_path, what, 1)
    three = _traced_kernel_names(tmp_path, what, 3)
    assert len(three) - len(one) == 2 * launches, (len(one), len(three))
    assert len([n for n in three if "moe_router_gemm" in n]) == 3, three
    assert len([n for n in three if "moe_route_align_one" in n]) == 3, three
    assert not [n for n in three if "moe_router_finish" in n], three
    report = os.environ.get("PETIT_ROUTE_TRACE_REPORT")
    if report:
        with open(report, "a") as f:
            f.write(f"{what}: {launches} launches per call: " + " | ".join(n[:60] for n in three[len(three) - launches:]) + "\n")

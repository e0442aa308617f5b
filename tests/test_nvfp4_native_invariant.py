"""The batch-invariant native-class GEMM on NVFP4 images (include/petit_amd.h "Batch-invariant native-class GEMM and MoE launch on NVFP4 images")
on the GPU: a row's bits do not move with m, its position or its neighbours; both forms equal the host twin and a float64 evaluation bit for
bit on inputs whose image, quantisation and partial sums are exact; the fold is the ascending one and the split form's slabs are the p_s;
quantised input equals 16-bit input; nothing is written outside C and the queried workspace; graph replay and repeated launches give the same
bits; random checkpoint-like weights stay inside the class's bound on the image's weights and the class tolerance on the true ones.
Shapes (n, k): (64, 1024): spans of 8 k-tiles, S = 4; (96, 768): spans of 2, three blocks of 32 rows (the whole form has a wave with one dead
block), S = 3; (128, 1536): spans of 4, S = 6; (64, 4352): S = 9, L = 512, last slice 256; gated: (128, 1024)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from petit_kernel import _lib
from test_gated_contract import expect as gated_expect
from test_gpu_parity import DEV, O, decode_qact, native_exact_bound, pk  # noqa: F401
from test_native_invariant_abi import BF16, FMTS, FP16, OK, dt, expect_plain, from16, host_quantize, to16
from test_nvfp4_native_invariant_abi import (E4M3_POW2, FP4, NV, SHAPES, build_image, exact_activations, exact_image, geometry, random_nvfp4, twin)

pytestmark = pytest.mark.gpu
GATED_SHAPE = (128, 1024)
SPLIT_M, WHOLE_M = 5, 70                       # one m of each form (the switch: m <= 64 split)
MS = (1, 2, 31, 32, 33, 64, 65, 200)
POISON = {True: 0x7FC1, False: 0x7E01}         # a NaN of the output type: no expected value is one
GUARD = 4096
L = _lib.lib
CASES = [(fmt, is_bf16) for fmt in FMTS for is_bf16 in (True, False)]
IDS = [f"{fmt}-{'bf16' if b else 'fp16'}" for fmt, b in CASES]
CLASS_COEF = {"mxfp8": 2e-2, "mxfp6": 2e-2, "mxfp4": 0.12}      # test_native_nvfp4_every_kernel's


def dev16(bits, is_bf16):
    return torch.from_numpy(bits.view(np.int16).copy()).view(dt(is_bf16)).to(DEV)


def out_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


@functools.lru_cache(maxsize=16)
def weights(n, k, kind):
    """-> (host image, the image's weights float64, the true NVFP4 weights float64, the image on the device), computed once per shape"""
    if kind == "exact":
        image, w = exact_image(n, k, 17)
        return image, w, w, image.to(DEV)
    q, s = random_nvfp4(n, k, 17)
    image, w = build_image(q, s)
    return image, w, O.dequant_nvfp4(q, s).astype(np.float64), image.to(DEV)


@functools.lru_cache(maxsize=16)
def random_rows(m, k, is_bf16, seed=31):
    return to16(np.random.default_rng([seed, m, k]).standard_normal((m, k)), is_bf16, exact=False)


def forms_ran(pk, n, k, is_bf16, ms):
    """through the queries: both forms are among `ms` (slabs S below the switch and 1 above; workspace on quantised input only in the split form)"""
    S, _ = geometry(n, k)
    split = [m for m in ms if pk.native_invariant_workspace_bytes(m, n, k, dt(is_bf16), "mxfp8", True) > 0]
    whole = [m for m in ms if m not in split]
    assert split and whole and max(split) == 64 and min(whole) == 65, (split, whole)
    assert all(pk.native_invariant_slabs(m, n, k, dt(is_bf16)) == S for m in split)
    assert all(pk.native_invariant_slabs(m, n, k, dt(is_bf16)) == 1 for m in whole)


# --- 1. invariance ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_a_rows_bits_do_not_move_with_m_or_position(pk, n, k, fmt, is_bf16):
    image = weights(n, k, "random")[3]
    rows = random_rows(200, k, is_bf16)
    gs = torch.tensor([0.37], dtype=torch.float32, device=DEV)
    bias = dev16(random_rows(1, n, is_bf16, seed=5)[0], is_bf16)
    full = out_bits(pk.mul_nvfp4_native_invariant(dev16(rows, is_bf16), image, gs, 200, n, k, fmt, bias))
    assert not np.isnan(from16(full, is_bf16)).any()
    probes = (3, 77, 199)
    forms_ran(pk, n, k, is_bf16, MS)
    for m in MS:
        order = np.arange(m)                                      # rows 0 .. m - 1 of the batch, with the probes at the first, a middle, the last position
        places = sorted({0, m // 2, m - 1})
        for p, r in zip(places, probes):
            order[p] = r
        got = out_bits(pk.mul_nvfp4_native_invariant(dev16(rows[order], is_bf16), image, gs, m, n, k, fmt, bias))
        for p, r in zip(places, probes):
            assert np.array_equal(got[p], full[r]), (m, p, r, int((got[p] != full[r]).sum()))


# --- 2. hostile neighbours -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_hostile_neighbours_do_not_reach_a_row(pk, fmt, is_bf16):
    n, k = 96, 768
    image = weights(n, k, "random")[3]
    probe_rows = random_rows(3, k, is_bf16, seed=41)
    alone = [out_bits(pk.mul_nvfp4_native_invariant(dev16(probe_rows[i:i + 1], is_bf16), image, None, 1, n, k, fmt))[0] for i in range(3)]
    big = 2.0 ** 120 if is_bf16 else 65504.0
    hostile = [np.nan, np.inf, -np.inf, big, -big, 0.0]
    for m in (20, 65):                                           # split, whole
        v = np.empty((m, k))
        for r in range(m):
            v[r] = hostile[r % len(hostile)]
        bits = to16(v, is_bf16, exact=False)
        places = (0, m // 2, m - 1)
        for p, i in zip(places, range(3)):
            bits[p] = probe_rows[i]
        got = out_bits(pk.mul_nvfp4_native_invariant(dev16(bits, is_bf16), image, None, m, n, k, fmt))
        for p, i in zip(places, range(3)):
            assert np.array_equal(got[p], alone[i]), (m, p)


# --- 3. the definition, bit for bit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layer", ["ops", "compiled"])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_both_forms_equal_the_twin_on_exact_inputs(pk, n, k, fmt, is_bf16, layer):
    """The image is exact (asserted on the CPU by exact_image: its dequant equals the oracle's dequant of the NVFP4 tensors), the quantiser is
    exact, every partial sum is exact: both forms equal the float64 product through the stated epilogue, and the host twin."""
    mul = getattr(pk, layer).mul_nvfp4_native_invariant
    image_h, w, _, image = weights(n, k, "exact")
    bias64 = np.random.default_rng(5).integers(-8, 9, n) * 0.5
    bias_bits = to16(bias64, is_bf16)
    for m in (SPLIT_M, WHOLE_M):
        a = exact_activations(m, k, 3)
        bits = to16(a, is_bf16)
        fold = a @ w.T
        assert (np.abs(a) @ np.abs(w).T).max() < 2 ** 22                 # every partial sum is exact, in any order
        qa_host = host_quantize(bits, is_bf16, fmt)
        assert np.array_equal(decode_qact(qa_host, m, k, fmt).astype(np.float64), a)      # the quantiser is exact
        for gs in (0.25, 1.0 / 3.0, None):
            for use_bias in (True, False):
                gsd = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=DEV)
                got = out_bits(mul(dev16(bits, is_bf16), image, gsd, m, n, k, fmt, dev16(bias_bits, is_bf16) if use_bias else None))
                gs32 = None if gs is None else float(np.float32(gs))
                want = expect_plain(fold.astype(np.float32), gs32, bias64 if use_bias else None, is_bf16)
                assert np.array_equal(got, want), (m, gs, use_bias, int((got != want).sum()))
                tw = twin(qa_host, image_h, gs32, bias_bits if use_bias else None, m, n, k, is_bf16, fmt)
                assert np.array_equal(got, tw), (m, gs, use_bias)


@pytest.mark.parametrize("act,name", [(1, "silu_mul"), (2, "swiglu_oai")])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_gated_epilogues_on_exact_inputs(pk, fmt, is_bf16, act, name):
    """y = fma(fold, gs, bias) with an exact fold, through the gated epilogue every gated kernel calls: held to the gated contract's band
    (tests/test_gated_contract.py: the device exponential is not the host's), and the two forms to each other bit for bit."""
    n, k = GATED_SHAPE
    _, w, _, image = weights(n, k, "exact")
    bias64 = np.random.default_rng(6).integers(-8, 9, n) * 0.125
    gs = 2.0 ** -7                                                    # (gate values of a few units: the activation is neither 0 nor the identity)
    a_rows = exact_activations(WHOLE_M, k, 9)
    per_row = {}
    for m in (SPLIT_M, WHOLE_M):
        a = a_rows[:m]
        y = (a @ w.T * gs + bias64[None, :]).astype(np.float32).astype(np.float64)        # one rounding: the fma
        P = gated_expect(types.SimpleNamespace(y=y), is_bf16, act)
        got = out_bits(pk.mul_nvfp4_native_invariant(dev16(to16(a, is_bf16), is_bf16), image, torch.tensor([gs], dtype=torch.float32, device=DEV), m, n,
                                                     k, fmt, dev16(to16(bias64, is_bf16), is_bf16), name))
        assert got.shape == (m, n // 2)
        assert not P.wrong(got).any(), (m, int(P.wrong(got).sum()))
        per_row[m] = got
    assert np.array_equal(per_row[SPLIT_M], per_row[WHOLE_M][:SPLIT_M])


# --- 4. fold order ---------------------------------------------------------------------------------------------------------------------------

def fold_problem(n, k, m, is_bf16):
    """Slices 0 and 1 hold +-BIG b against the same weights (p_1 = -p_0 exactly), the others SMALL integers: only the ascending fold keeps the
    small slices' sum, ((p_0 + p_1) + p_2) + ... ; any other order rounds it against a BIG partial sum first.  Group scales 1: the image is exact."""
    S, Lk = geometry(n, k)
    assert S >= 3
    rng = np.random.default_rng([n, k, 99])
    code = rng.integers(0, 16, (n, k), dtype=np.uint8)
    code[:, Lk:2 * Lk] = code[:, :Lk]
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    image, w = build_image(q, np.full((n, k // 16), E4M3_POW2[0], dtype=np.uint8))
    assert np.array_equal(w, FP4[code])
    big, small = (2.0 ** 24, 1.0) if is_bf16 else (2.0 ** 13, 2.0 ** -10)
    v = np.array([0.0, 1, 2, 3, 4, 6])[rng.integers(0, 6, (m, k // 32, 32))]
    v[:, :, 0] = np.array([4.0, 6.0])[rng.integers(0, 2, (m, k // 32))]
    v = (v * rng.choice([-1.0, 1.0], v.shape)).reshape(m, k)
    v[:, Lk:2 * Lk] = -v[:, :Lk]
    a = v * small
    a[:, :2 * Lk] = v[:, :2 * Lk] * big
    parts = [a[:, s * Lk:min(k, (s + 1) * Lk)] @ w[:, s * Lk:min(k, (s + 1) * Lk)].T for s in range(S)]
    for p in parts:
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)                  # every p_s is an fp32 number
    return image, a, parts


def fold32(parts, order):
    acc = parts[order[0]].astype(np.float32)
    for s in order[1:]:
        acc = (acc + parts[s].astype(np.float32)).astype(np.float32)
    return acc


@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_the_fold_is_ascending_and_the_slabs_are_the_partial_sums(pk, n, k, fmt, is_bf16):
    S, Lk = geometry(n, k)
    a_type = BF16 if is_bf16 else FP16
    for m in (SPLIT_M, WHOLE_M):
        image_h, a, parts = fold_problem(n, k, m, is_bf16)
        image = image_h.to(DEV)
        want = expect_plain(fold32(parts, list(range(S))), None, None, is_bf16)
        others = expect_plain(fold32(parts, list(range(S))[::-1]), None, None, is_bf16)
        assert (want != others).mean() > 0.25                                              # the inputs tell the orders apart
        bits = to16(a, is_bf16)
        got = out_bits(pk.mul_nvfp4_native_invariant(dev16(bits, is_bf16), image, None, m, n, k, fmt))
        assert np.array_equal(got, want), (m, int((got != want).sum()))
        if m == SPLIT_M:                                                                   # the slabs, through the C ABI on quantised bytes
            qa = pk.quantize_activations(dev16(bits, is_bf16), fmt)
            nbytes = int(L.petit_gemm_native_invariant_workspace_bytes(m, n, k, a_type, FMTS[fmt], 1))
            assert nbytes == (S * m * n * 4 + 255) // 256 * 256
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
            c = torch.empty(m, n, dtype=dt(is_bf16), device=DEV)
            hints = _lib.SolutionHints(a_type, NV, a_type, 0)
            rc = L.petit_gemm_nvfp4_native_invariant(c.data_ptr(), qa.data.data_ptr(), image.data_ptr(), None, m, n, k, C.byref(hints), FMTS[fmt], 1,
                                                     None, ws.data_ptr(), None)
            assert rc == OK
            torch.cuda.synchronize()
            slabs = ws[: S * m * n * 4].view(torch.float32).reshape(S, m, n).cpu().numpy()
            for sl in range(S):
                assert np.array_equal(slabs[sl].astype(np.float64), parts[sl]), sl
            assert np.array_equal(out_bits(c), want)


# --- 5. accuracy -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_accuracy_on_checkpoint_like_weights(pk, n, k, fmt, is_bf16):
    """(1) per output, the class's derived bound (tests/test_gpu_parity.py native_exact_bound, next to the usual 1e-2 band) against the oracle on
    (CPU-quantised activations, the image's weights); (2) the class tolerance against the oracle on the TRUE NVFP4 weights, widened by the
    header's re-encoding bound: the tolerances of test_native_nvfp4_every_kernel, no new numbers."""
    _, w6, dq, image = weights(n, k, "random")
    q, s = random_nvfp4(n, k, 17)
    _, sb = O.nv6_reencode(q, s)
    wb = np.maximum(2.0 ** -4 * np.abs(dq), np.repeat(np.ldexp(1.0, sb.astype(np.int64) - 127 - 4), 32, axis=1))
    gs = 0.0123
    g32 = float(np.float32(gs))
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    for m in (8, WHOLE_M):
        bits = random_rows(m, k, is_bf16, seed=77)
        a = from16(bits, is_bf16)
        a_q = decode_qact(host_quantize(bits, is_bf16, fmt), m, k, fmt).astype(np.float64)
        got = from16(out_bits(pk.mul_nvfp4_native_invariant(dev16(bits, is_bf16), image, gsd, m, n, k, fmt)), is_bf16)
        exact = a_q @ w6.T * g32
        derived = native_exact_bound(a_q.astype(np.float32), w6.astype(np.float32), g32, fmt)
        err = np.abs(got - exact)
        assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)).all(), (m, float(err.max()))
        full, sum_abs, w_term = a @ dq.T * g32, np.abs(a) @ np.abs(dq).T * g32, np.abs(a) @ wb.T * g32
        assert (np.abs(got - full) <= CLASS_COEF[fmt] * sum_abs + w_term + 1e-2).all(), m


# --- 6. pre-quantised input ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_quantised_input_gives_the_bits_of_the_16_bit_path(pk, fmt, is_bf16):
    n, k = 128, 1536
    image = weights(n, k, "random")[3]
    gsd = torch.tensor([1.5], dtype=torch.float32, device=DEV)
    for m in (7, WHOLE_M):
        x = dev16(random_rows(m, k, is_bf16, seed=61), is_bf16)
        on16 = pk.mul_nvfp4_native_invariant(x, image, gsd, m, n, k, fmt)
        qa = pk.quantize_activations(x, fmt)
        assert isinstance(qa, pk.QuantizedActivations) and qa.fmt == fmt
        for layer in (pk.ops, pk.compiled):
            got = layer.mul_nvfp4_native_invariant(qa, image, gsd, m, n, k, fmt)
            assert torch.equal(got.view(torch.int16), on16.view(torch.int16)), m
        other = "mxfp4" if fmt != "mxfp4" else "mxfp8"
        with pytest.raises(RuntimeError, match="quantised activations are"):
            pk.mul_nvfp4_native_invariant(qa, image, gsd, m, n, k, other)


# --- 7. write contract -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quantized", [0, 1])
@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_every_output_is_written_and_nothing_else(pk, fmt, is_bf16, quantized):
    n, k = 96, 768
    _, w, _, image = weights(n, k, "exact")
    a_type = BF16 if is_bf16 else FP16
    hints = _lib.SolutionHints(a_type, NV, a_type, 0)
    for m in (1, 33, 65):
        a = exact_activations(m, k, 13)
        bits = to16(a, is_bf16)
        ad = dev16(bits, is_bf16)
        src = pk.quantize_activations(ad, fmt).data if quantized else ad
        nbytes = int(L.petit_gemm_native_invariant_workspace_bytes(m, n, k, a_type, FMTS[fmt], quantized))
        assert (nbytes > 0) == (m <= 64 or not quantized)
        ws = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)         # exactly the queried bytes between two guards
        cbuf = torch.full((m * n + GUARD,), POISON[is_bf16], dtype=torch.int16, device=DEV).view(torch.int16)
        c = cbuf[GUARD // 2: GUARD // 2 + m * n]
        assert c.data_ptr() % 16 == 0 and (ws.data_ptr() + GUARD) % 256 == 0 and image.data_ptr() % 256 == 0
        rc = L.petit_gemm_nvfp4_native_invariant(c.data_ptr(), src.data_ptr(), image.data_ptr(), None, m, n, k, C.byref(hints), FMTS[fmt], quantized,
                                                 None, (ws.data_ptr() + GUARD) if nbytes else None, None)
        assert rc == OK
        torch.cuda.synchronize()
        got = c.cpu().numpy().view(np.uint16).reshape(m, n)
        assert np.array_equal(got, expect_plain((a @ w.T).astype(np.float32), None, None, is_bf16))      # every output, and none is the poison
        guard = cbuf.cpu().numpy().view(np.uint16)
        assert (guard[: GUARD // 2] == POISON[is_bf16]).all() and (guard[GUARD // 2 + m * n:] == POISON[is_bf16]).all()
        wsh = ws.cpu().numpy()
        assert (wsh[:GUARD] == 0xA5).all() and (wsh[GUARD + nbytes:] == 0xA5).all()


# --- 8. graph and repeat ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,is_bf16", CASES, ids=IDS)
def test_graph_replay_and_repeated_launches(pk, fmt, is_bf16):
    n, k = 64, 1024
    image = weights(n, k, "random")[3]
    gsd = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    for m in (8, WHOLE_M):
        ad = dev16(random_rows(m, k, is_bf16, seed=81), is_bf16)
        first = pk.ops.mul_nvfp4_native_invariant(ad, image, gsd, m, n, k, fmt).clone()
        for _ in range(10):
            again = pk.ops.mul_nvfp4_native_invariant(ad, image, gsd, m, n, k, fmt)
            assert torch.equal(again.view(torch.int16), first.view(torch.int16))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = pk.ops.mul_nvfp4_native_invariant(ad, image, gsd, m, n, k, fmt)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int16), first.view(torch.int16)), m

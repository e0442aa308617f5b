"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (via petit_kernel.ops,
which is a ctypes shim), against the CPU oracle, the committed golden vectors and
size-independent properties at BASELINE.json's full sizes.

Tolerances
  * repack: bit exact (byte movement).
  * dequant (identity-activation GEMM): bit exact -- fp4 x scale needs <= 5 significant bits.
  * GEMM: |c - ref| <= max(1e-2, 1e-2 * |ref|), the reference's own gtest bound
    (fp4/gemm_fp4_fp16_rocm_test.cc:36,53) and BASELINE.json's "within 1e-2 rel-err"; the
    reference's pytest uses the looser rtol = atol = 2e-2 (tests/ops/test_fp4_gemm_quark.py:54).
"""
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent

from oracle import cdna4_layout as LY
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    name = torch.cuda.get_device_properties(0).gcnArchName
    assert name.startswith("gfx950"), f"these kernels are gfx950 code objects, device is {name}"
    return petit_kernel


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(b: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(b.view(np.int16).copy()).view(dtype)


def to_f32(b: np.ndarray, is_bf16: bool) -> np.ndarray:
    return O.bf16_bits_to_f32(b) if is_bf16 else O.f16_bits_to_f32(b)


def check_gemm(c_bits, ref_f32, is_bf16, sum_abs=None, sum_abs_coef=1e-5):
    """sum_abs: optional sum_k |a||w| per output.  With e8m0 block scales the products span many
    binades, and ANY f32-accumulating implementation carries ~sqrt(K)*2^-24 of that sum as absolute
    error; where the true result cancels to ~0 that, not 1e-2, is the honest bound."""
    c = to_f32(c_bits, is_bf16).astype(np.float64)
    ref = ref_f32.astype(np.float64)
    fin = np.isfinite(ref) & (np.abs(ref) < (3.0e38 if is_bf16 else 6.0e4))
    err = np.abs(c - ref)
    bound = np.maximum(1e-2, 1e-2 * np.abs(ref))
    if sum_abs is not None:
        bound = np.maximum(bound, sum_abs_coef * sum_abs)
    assert np.isfinite(c[fin]).all()
    if not (err[fin] <= bound[fin]).all():
        ratio = np.where(fin, err / bound, 0.0)
        w = np.unravel_index(ratio.argmax(), ratio.shape)
        raise AssertionError(f"{int((ratio > 1).sum())} of {ratio.size} outputs out of bound; worst at {w}: got {c[w]!r} ref {ref[w]!r} "
                             f"err {err[w]:.4g} bound {bound[w]:.4g}" + (f" sum|a||w| {sum_abs[w]:.4g}" if sum_abs is not None else "")
                             + f"; largest err {err[fin].max():.4g} at ref {ref[fin][err[fin].argmax()]:.4g}")
    # and much tighter on average: one 16-bit rounding of an f32-accumulated sum
    rel = err[fin] / np.maximum(np.abs(ref[fin]), 1e-3)
    assert np.median(rel) < (2 ** -8 if is_bf16 else 2 ** -11)


def run_case(pk, kind, a_bits, is_bf16, q, s, gs, m, n, k, solution_id=-1):
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a = from_bits(a_bits, dtype).to(DEV)
    qd = torch.from_numpy(q).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    if kind == "nv":
        b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
        sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        c = pk.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, solution_id)
    else:
        b = pk.repack_mxfp4(qd.view(torch.int32), n, k)
        sp = pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        c = pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, solution_id)
    torch.cuda.synchronize()
    assert c.shape == (m, n) and c.dtype == dtype and c.is_cuda
    return bits(c)


# --- repack: bit exact against the layout model --------------------------------------

@pytest.mark.parametrize("n,k", [(16, 256), (64, 256), (128, 512), (96, 768), (256, 1024), (8192, 8192)])
def test_repack_bit_exact(pk, n, k):
    rng = np.random.default_rng(n + k)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    s = rng.integers(0, 256, (n, k // 16), dtype=np.uint8)
    mx = rng.integers(0, 256, (n, k // 32), dtype=np.uint8)
    b = pk.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    assert b.shape == (n // 16, 2 * k) and b.dtype == torch.int32            # fp4.cc:62-63
    want = LY.pack_weights(q.view(np.uint32).reshape(n, k // 8))
    assert np.array_equal(b.cpu().numpy().view(np.uint32).ravel(), want)
    sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    assert sp.shape == (n, k // 16) and sp.dtype == torch.float8_e4m3fn       # fp4.cc:101-107
    assert np.array_equal(sp.view(torch.uint8).cpu().numpy().ravel(), LY.pack_nvscales(s, k))
    if n % 32 == 0:
        mp = pk.process_mxfp4_scales(torch.from_numpy(mx).to(DEV), n, k)
        assert mp.shape == (n // 32, k) and mp.dtype == torch.uint8          # fp4.cc:142-148
        assert np.array_equal(mp.cpu().numpy().ravel(), LY.pack_mxscales(mx, k))
    # repack_mxfp4 is the same weight shuffle (petit_kernel/__init__.py:27-28)
    b2 = pk.repack_mxfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    assert torch.equal(b, b2)


@pytest.mark.parametrize("kind", ["nv", "mx"])
def test_dense_dequant_debug_op(pk, golden_dir, kind):
    """petit_dequant_packed_weights (the reference keeps DequantPetitFp4 / DequantPetitMxFp4 for the same purpose,
    quantization_utils.cu:542-727): packed weights + packed scales -> dense f32, BIT EXACT against the oracle's
    dequant on random data and on the exhaustive code x scale tables; bf16 / fp16 outputs are one RNE rounding of it."""
    n, k = 96 if kind == "nv" else 64, 1024
    _, q, s, _ = random_problem(kind, 1, n, k, 606, True)
    if kind == "nv":
        s = ((np.arange(n)[:, None] * 7 + np.arange(k // 16)[None, :]) % 126 + 1).astype(np.uint8)     # every positive e4m3 scale
    else:
        s = ((np.arange(n)[:, None] * 29 + np.arange(k // 32)[None, :]) % 237 + 1).astype(np.uint8)    # e8m0 1..237
    qd = torch.from_numpy(q).to(DEV).view(torch.int32)
    if kind == "nv":
        b, sp = pk.repack_nvfp4(qd, n, k), pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        want = O.dequant_nvfp4(q, s)
    else:
        b, sp = pk.repack_mxfp4(qd, n, k), pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        want = O.dequant_mxfp4(q, s)
    got = pk.ops.dequant_packed(b, sp, n, k, "nvfp4" if kind == "nv" else "mxfp4")
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    g16 = pk.ops.dequant_packed(b, sp, n, k, "nvfp4" if kind == "nv" else "mxfp4", torch.bfloat16)
    assert np.array_equal(bits(g16), O.f32_to_bf16_bits(want))                      # exact: <= 5 significant bits
    scaled = pk.ops.dequant_packed(b, sp, n, k, "nvfp4" if kind == "nv" else "mxfp4", torch.float32, 0.75)
    assert np.array_equal(scaled.cpu().numpy(), want * np.float32(0.75))


# --- exhaustive dequant truth tables through the GEMM, bit exact ----------------------

@pytest.mark.parametrize("is_bf16", [True, False])
def test_exhaustive_nv_dequant_bit_exact(pk, golden_dir, is_bf16):
    """16 codes x every positive e4m3 scale (ExhaustiveFp4DequantTest,
    quantization_utils_fp4_test.cc:344-365) extracted with identity activations:
    C[m][n] = W[n][m], one non-zero product per output, so the result must be exact."""
    n, k = 128, 256
    t = np.load(golden_dir / "dequant_tables.npz")["nv"]        # [16 codes, 126 scales]
    code = np.arange(n)[:, None] % 16 * np.ones((1, k), dtype=np.int64)
    code = (code + np.arange(k)[None, :]) % 16                  # every code in every nibble slot
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    sidx = (np.arange(n)[:, None] * 16 + np.arange(k // 16)[None, :]) % 126
    s = (1 + sidx).astype(np.uint8)
    want = t[code, np.repeat(sidx, 16, axis=1)]                 # f32 [n, k]
    eye = np.eye(k, dtype=np.float32)
    a_bits = O.f32_to_bf16_bits(eye) if is_bf16 else eye.astype(np.float16).view(np.uint16)
    c = run_case(pk, "nv", a_bits, is_bf16, q, s, 1.0, k, n, k)
    got = to_f32(c, is_bf16)                                    # [k, n] = W^T
    assert np.array_equal(got.T, want)


@pytest.mark.parametrize("is_bf16", [True, False])
def test_exhaustive_mx_dequant_bit_exact(pk, golden_dir, is_bf16):
    """16 codes x e8m0 1..237 with the reference's row/col-mixing scale generator
    (MxFp4DequantTest, quantization_utils_fp4_test.cc:266-278,311-342)."""
    n, k = 256, 256
    t = np.load(golden_dir / "dequant_tables.npz")["mx"]        # [16, 237]
    code = (np.arange(n)[:, None] + np.arange(k)[None, :]) % 16
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    sidx = (np.arange(k // 32)[None, :] + 29 * np.arange(n)[:, None]) % 237
    s = (1 + sidx).astype(np.uint8)
    want = t[code, np.repeat(sidx, 32, axis=1)]
    eye = np.eye(k, dtype=np.float32)
    a_bits = O.f32_to_bf16_bits(eye) if is_bf16 else eye.astype(np.float16).view(np.uint16)
    c = run_case(pk, "mx", a_bits, is_bf16, q, s, 1.0, k, n, k)
    if is_bf16:
        assert np.array_equal(to_f32(c, True).T, want)
    else:
        # fp16 output: 2^(e-127) leaves the fp16 range for most of 1..237 -- the single f32 -> fp16
        # rounding (to inf / subnormal / zero) must be the IEEE one, bit for bit
        with np.errstate(over="ignore"):
            want16 = want.astype(np.float16)
        assert np.array_equal(c.view(np.float16).T == 0, want16 == 0)
        nz = want16 != 0
        assert np.array_equal(c.T[nz], want16.view(np.uint16)[nz])


# --- the reference's pytest cases, from the committed golden vectors ------------------

@pytest.mark.parametrize("name", ["nv_64_128_256_1234", "nv_96_64_512_2026",
                                  "nv_64_128_256_1234_f16", "nv_96_64_512_2026_f16"])
def test_nv_golden_cases(pk, golden_dir, name):
    g = np.load(golden_dir / f"{name}.npz")
    m, k = g["a"].shape
    n = g["q"].shape[0]
    is_bf16 = bool(g["a_is_bf16"])
    c = run_case(pk, "nv", g["a"], is_bf16, g["q"], g["s"], float(g["gs"][0]), m, n, k)
    check_gemm(c, to_f32(g["c_ref"], is_bf16), is_bf16)
    # the reference pytest's own criterion (tests/ops/test_fp4_gemm_quark.py:54)
    torch.testing.assert_close(torch.from_numpy(to_f32(c, is_bf16)), torch.from_numpy(to_f32(g["c_ref"], is_bf16)),
                               rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("name", ["mx_64_128_256_1234", "mx_96_96_512_2026",
                                  "mx_64_128_256_1234_f16", "mx_96_96_512_2026_f16"])
def test_mx_golden_cases(pk, golden_dir, name):
    g = np.load(golden_dir / f"{name}.npz")
    m, k = g["a"].shape
    n = g["q"].shape[0]
    is_bf16 = bool(g["a_is_bf16"])
    c = run_case(pk, "mx", g["a"], is_bf16, g["q"], g["s"], float(g["gs"][0]), m, n, k)
    ref = to_f32(g["c_ref"], is_bf16)
    got = to_f32(c, is_bf16)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)          # overflow to inf in the same places
    assert np.array_equal(np.sign(got[~fin]), np.sign(ref[~fin]))
    if fin.any():   # e8m0 1..237 against fp16: every output of a case may overflow
        rel = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-30)
        assert rel.max() <= 1e-2


def test_config1_golden(pk, golden_dir):
    """BASELINE.json configs[0] (M=1, N=K=4096) against the reference-produced c_ref."""
    from test_oracle import config1_inputs
    g = np.load(golden_dir / "config1_nv_1_4096_4096.npz")
    a, q, s, gs = config1_inputs()
    c = run_case(pk, "nv", a, True, q, s, float(gs), 1, 4096, 4096)
    check_gemm(c, to_f32(g["c_ref"], True), True)


# --- seeded random problems against the oracle: shapes, dtypes, every solution ---------

def random_problem(kind, m, n, k, seed, is_bf16, mx_band=None):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, k), dtype=np.float32)
    a_bits = O.f32_to_bf16_bits(a) if is_bf16 else a.astype(np.float16).view(np.uint16)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    if kind == "nv":
        sf = rng.random((n, k // 16), dtype=np.float32) * 3.5 + 0.25
        s = torch.from_numpy(sf).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    else:
        lo, hi = mx_band or (119, 136)
        s = rng.integers(lo, hi, (n, k // 32), dtype=np.uint8)
    gs = float(rng.random() * 1.5 + 0.5)
    return a_bits, q, s, gs


def oracle_ref(kind, a_bits, is_bf16, q, s, gs):
    dq = O.dequant_nvfp4(q, s) if kind == "nv" else O.dequant_mxfp4(q, s)
    _, cf = O.gemm_ref(a_bits, is_bf16, dq, gs)
    return cf


def oracle_sum_abs(kind, a_bits, is_bf16, q, s, gs):
    if kind != "mx":
        return None
    dq = np.abs(O.dequant_mxfp4(q, s))
    a = np.abs(to_f32(a_bits, is_bf16))
    return (a @ dq.T) * gs


SHAPES = [
    # (m, n, k): ragged M, N % 16 only, every span size (K % 1024 / 512 / 256)
    (1, 16, 256), (1, 64, 1024), (3, 48, 512), (7, 80, 768), (16, 128, 2048), (17, 64, 1024),
    (33, 96, 1024), (64, 64, 2048), (100, 32, 256), (5, 4096, 4096), (130, 256, 1024),
    (512, 1024, 2048), (257, 144, 768),      # the tiled large-M kernel, ragged M and N
]


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_random_vs_oracle_default_solution(pk, kind, is_bf16, m, n, k):
    if kind == "mx" and n % 32:
        pytest.skip("MX scale tensor contract needs N % 32 (fp4.cc:145-147)")
    a, q, s, gs = random_problem(kind, m, n, k, 1000 + m + n + k, is_bf16)
    c = run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k)
    check_gemm(c, oracle_ref(kind, a, is_bf16, q, s, gs), is_bf16, oracle_sum_abs(kind, a, is_bf16, q, s, gs))


# shapes NO table knows, each within reach of a tabulated one (pick.hip kNearestMaxDistance): solution_id = -1 runs the kernel the arch table names
# for the NEAREST tabulated shape (hal.hip tuned_nearest) -- kernels picked for another N / K, K splits sized for another span count, 224- and
# 320-column tiles on an N they do not divide
UNSEEN_SHAPES = [(1, 5152, 5120), (8, 7232, 2304), (16, 4192, 13312), (24, 8160, 7936), (32, 10400, 8704), (48, 3616, 4352), (64, 8192, 7168),
                 (96, 2496, 7424), (128, 6176, 3840), (200, 14560, 5120), (256, 28704, 4096), (384, 4160, 4864), (512, 7200, 8192)]


@pytest.mark.parametrize("m,n,k", UNSEEN_SHAPES)
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_default_solution_on_unseen_shapes_near_the_table(pk, kind, is_bf16, m, n, k):
    from petit_kernel import _lib
    import ctypes as C
    dt = _lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16
    hints = _lib.SolutionHints(dt, _lib.CXX_DTYPE_FP4_E2M1 if kind == "nv" else _lib.CXX_DTYPE_MXFP4_E2M1, dt, 0)
    assert _lib.lib.petit_gemm_default_solution(C.byref(hints), m, n, k) != 0
    a, q, s, gs = random_problem(kind, m, n, k, 77 + m + n + k, is_bf16)
    c = run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k)
    check_gemm(c, oracle_ref(kind, a, is_bf16, q, s, gs), is_bf16, oracle_sum_abs(kind, a, is_bf16, q, s, gs))


MX_F16_PROBLEMS = [(1, 256, 2048), (3, 96, 512), (8, 160, 1024), (16, 288, 1024), (40, 64, 3072), (64, 128, 2048), (130, 256, 1024), (300, 512, 768),
                   (2, 4128, 4096), (512, 1024, 2048), (16, 512, 8192), (256, 256, 4096)]


def mx_f16_scale_profiles(n, k, seed):
    """MXFP4 scale tensors that drive the fp16 x MXFP4 kernels (Fp16Mx, csrc/device_common.hpp) through each of their bodies, with the global
    scale that brings the outputs to O(1) (the parity bound has an absolute floor of 1e-2: tiny outputs would pass vacuously):
      fast      every byte in 114..140, both ends present: the single-MFMA fp16 body everywhere
      fallback  every byte in 96..113: the exact bf16 hi / lo body from the first span on
      switch    in range, with a sprinkle of bytes just outside it (100..113, 141..143) placed in the SECOND half of K for the even 16-row
                tiles and anywhere for a few others: waves start in the fast body and switch at different spans, neighbours never do"""
    rng = np.random.default_rng(seed)
    kb = k // 32
    fast = rng.integers(114, 141, (n, kb), dtype=np.uint8)
    fast[0, 0], fast[-1, -1] = 114, 140
    fallback = rng.integers(96, 114, (n, kb), dtype=np.uint8)
    switch = rng.integers(128, 141, (n, kb), dtype=np.uint8)
    for t in range(0, n // 16, 2):          # even tiles: one odd byte somewhere in the second half of K
        switch[16 * t + rng.integers(0, 16), kb // 2 + rng.integers(0, max(1, kb - kb // 2))] = rng.choice([100, 113, 141, 143])
    for t in rng.integers(0, n // 16, max(1, n // 64)):   # a few tiles: odd bytes anywhere (incl. the very first block)
        switch[16 * t + rng.integers(0, 16), rng.integers(0, kb)] = rng.choice([112, 142])
    switch[5 % n, 0] = 141
    return {"fast": (fast, 2.0 ** -12), "fallback": (fallback, 2.0 ** 13), "switch": (switch, 2.0 ** -13)}


@pytest.mark.parametrize("m,n,k", MX_F16_PROBLEMS)
def test_fp16_mxfp4_every_solution_fast_fallback_switch(pk, m, n, k):
    """fp16 x MXFP4 decides in the kernel, per wave and span, between the single-MFMA fp16 body (scale bytes 114..140) and the exact fallback
    for any e8m0 scale -- no caller promise, no tensor mark.  Every enumerated kernel and the default pick against the oracle on scale
    profiles that keep every wave in the fast body, put every wave in the fallback, and make waves switch at different spans."""
    a, q, _, _ = random_problem("mx", m, n, k, 4242 + m + n + k, False)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.float16
    h.b_type = pk.DataType.mxfloat4_e2m1
    sols = pk.ops.get_fp4_solutions(h, m, n, k)
    assert sols and all((sid >> 28) & 0xF == 2 for sid in sols)
    assert any((sid >> 48) & 0xF == 12 for sid in sols) or k % 1024 or m < 1      # the 32x32x16 kernels exist for this family now
    for name, (s, gs) in mx_f16_scale_profiles(n, k, 77 + n + k).items():
        ref = oracle_ref("mx", a, False, q, s, gs)
        sum_abs = oracle_sum_abs("mx", a, False, q, s, gs)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0.05, name   # the check below is not vacuous
        for sid in [-1] + list(sols):
            try:
                check_gemm(run_case(pk, "mx", a, False, q, s, gs, m, n, k, sid), ref, False, sum_abs)
            except AssertionError as e:
                raise AssertionError(f"profile {name}, solution {sid:#x}: {e}") from None
        for splitk in (2, 4):   # K splits across workgroups: the slices start in different spans
            for sid in sols:
                if (sid >> 48) & 0xF in (0, 8, 12) and k // (128 * (8 if k % 1024 == 0 else 4 if k % 512 == 0 else 2)) >= splitk:
                    sk = (sid & ~(0xF << 60)) | (splitk << 60)
                    try:
                        check_gemm(run_case(pk, "mx", a, False, q, s, gs, m, n, k, sk), ref, False, sum_abs)
                    except AssertionError as e:
                        raise AssertionError(f"profile {name}, solution {sk:#x}: {e}") from None
                    break


def test_fp16_mxfp4_no_promise_no_mark(pk):
    """What round 3 got wrong, pinned: nothing about the fast path hangs on the Python tensor object.  nn.Parameter-wrapped scales, a clone,
    and a scale tensor OVERWRITTEN IN PLACE with out-of-range values all give the oracle's result; the deprecated b_type 8 and the tuner's
    old kind name are plain MXFP4; process_mxfp4_scales attaches nothing and does not look at the values."""
    m, n, k = 16, 256, 4096
    a, q, s_in, _ = random_problem("mx", m, n, k, 99, False, mx_band=(118, 137))
    gs = 2.0 ** -6
    ad = from_bits(a, torch.float16).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    b = pk.repack_mxfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = pk.process_mxfp4_scales(torch.from_numpy(s_in).to(DEV), n, k)
    assert not hasattr(sp, "petit_scales_in_fp16_range")
    ref_in = oracle_ref("mx", a, False, q, s_in, gs)
    c0 = pk.mul_mxfp4_a16(ad, b, sp, gsd, m, n, k, -1)
    check_gemm(bits(c0), ref_in, False, oracle_sum_abs("mx", a, False, q, s_in, gs))
    for alias in (torch.nn.Parameter(sp, requires_grad=False), sp.clone(), sp.data):
        assert torch.equal(pk.mul_mxfp4_a16(ad, b, alias, gsd, m, n, k, -1), c0)
    # weight hot-swap into the SAME tensor object: scales far outside fp16's range (2^-37 .. 2^-17), outputs brought back by the global scale
    s_out = np.random.default_rng(5).integers(90, 111, (n, k // 32), dtype=np.uint8)
    sp.copy_(pk.process_mxfp4_scales(torch.from_numpy(s_out).to(DEV), n, k))
    gs2 = 2.0 ** 22
    ref_out = oracle_ref("mx", a, False, q, s_out, gs2)
    assert np.abs(ref_out).max() > 0.05
    c1 = pk.mul_mxfp4_a16(ad, b, sp, torch.tensor([gs2], dtype=torch.float32, device=DEV), m, n, k, -1)
    check_gemm(bits(c1), ref_out, False, oracle_sum_abs("mx", a, False, q, s_out, gs2))
    # the deprecated dtype value is an alias at the C ABI (hints.b_type = 8) ...
    h7, h8 = pk.PetitSolutionHints(), pk.PetitSolutionHints()
    for h, bt in ((h7, pk.DataType.mxfloat4_e2m1), (h8, pk.DTYPE_MXFP4_E2M1_F16RANGE)):
        h.a_type = h.c_type = torch.float16
        h.b_type = bt
    assert pk.ops.get_fp4_solutions(h7, m, n, k) == pk.ops.get_fp4_solutions(h8, m, n, k)
    assert pk.ops.resolve_solution(h7, m, n, k) == pk.ops.resolve_solution(h8, m, n, k) != 0
    # ... and so is the tuner's old kind name
    sid, us = pk.tune_tensors(ad, (b, sp), gsd, m, n, k, kind="mxfp4_f16range", persist=False, rotate_mb=16)
    assert (sid >> 28) & 0xF == 2 and us > 0
    assert pk.mxfp4_scales_in_fp16_range(torch.from_numpy(s_in).to(DEV)) and not pk.mxfp4_scales_in_fp16_range(torch.from_numpy(s_out).to(DEV))


@pytest.mark.parametrize("m,n,k", [(1, 256, 2048), (16, 272, 1024), (40, 64, 3072), (9, 96, 512), (2, 32, 256), (7, 96, 2048),
                                   (3, 48, 512), (4, 80, 1536), (1, 48, 768), (2, 4128, 4096)])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_every_solution_vs_oracle(pk, kind, is_bf16, m, n, k):
    """The counterpart of the reference's one-gtest-per-tile-shape list
    (fp4/gemm_fp4_fp16_rocm_test.cc:343-381): every enumerated kernel, same inputs."""
    if kind == "mx" and n % 32:
        pytest.skip("MX scale tensor contract needs N % 32")
    a, q, s, gs = random_problem(kind, m, n, k, 77 + m + n + k, is_bf16)
    ref = oracle_ref(kind, a, is_bf16, q, s, gs)
    sum_abs = oracle_sum_abs(kind, a, is_bf16, q, s, gs)
    h = pk.PetitSolutionHints()
    h.a_type = torch.bfloat16 if is_bf16 else torch.float16
    h.c_type = h.a_type
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    sols = pk.ops.get_fp4_solutions(h, m, n, k)
    assert sols
    for sid in sols:
        c = run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k, sid)
        check_gemm(c, ref, is_bf16, sum_abs)


BATCH_PROBLEMS = [(33, 272, 4096), (64, 96, 8192), (100, 160, 3072), (128, 64, 2048), (17, 48, 1536), (40, 64, 768), (130, 288, 5120), (44, 10240, 1024)]


@pytest.mark.parametrize("m,n,k", BATCH_PROBLEMS)
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_batch_kernels_every_shape_and_split(pk, kind, is_bf16, m, n, k):
    """csrc/gemm_batch.hpp (17 <= M <= 128, round 5): every instance x cross-workgroup K split 1 / 2 / 4 on problems that exercise what is new in
    it -- several m-blocks with a ragged last one, K ranges that do not divide over the WK parts x the slices (parts that idle through their
    partners' barriers), every span size (K % 1024 / 512 / 256), ragged N, one wide N -- against the oracle, and every launch repeated: the counted
    vmcnt + bare s_barrier protocol and the LDS reduction are deterministic by design, so any bit difference between two launches is a race."""
    if kind == "mx" and n % 32:
        n += 16          # the MX scale tensor contract needs N % 32
    a, q, s, gs = random_problem(kind, m, n, k, 4242 + m + n + k, is_bf16)
    ref = oracle_ref(kind, a, is_bf16, q, s, gs)
    sum_abs = oracle_sum_abs(kind, a, is_bf16, q, s, gs)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    batch = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF == 0 and (sid >> 36) & 0xF == 2]
    assert len(batch) >= 2 and any((sid >> 21) & 7 for sid in batch), "the loader-wave form"
    assert any((sid >> 21) & 7 == 0 for sid in batch) or (kind == "mx" and not is_bf16), "the form without a loader wave (fp16 x MXFP4 has the loader-wave form only)"
    ran = 0
    for sid in batch:
        for splitk in (1, 2, 4):
            sk = (sid & ~(0xF << 60)) | (splitk << 60)
            first = run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k, sk)
            check_gemm(first, ref, is_bf16, sum_abs)
            for _ in range(2):
                assert np.array_equal(run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k, sk), first), f"{sk:#x}: launches differ"
            ran += 1
    assert ran == 3 * len(batch)


# The problem sizes of the reference's own GEMM gtest list (fp4/gemm_fp4_fp16_rocm_test.cc:333-425): each
# TEST_BF16(m, n, k, ...) runs TestGemm(m, lcm(n, 32), lcm(k, 256)); de-duplicated.  Its per-case tile shapes
# have no meaning here -- every kernel this build enumerates for the problem is run instead.
REFERENCE_GTEST_PROBLEMS = [
    (16, 32, 256), (16, 32, 512), (16, 64, 256), (16, 64, 512), (16, 128, 256), (32, 32, 256), (32, 32, 512),
    (32, 64, 256), (32, 64, 512), (32, 128, 256), (64, 32, 256), (64, 64, 256), (64, 96, 256), (64, 128, 256),
    (80, 128, 256), (96, 64, 256), (96, 96, 256), (128, 64, 256), (128, 128, 256), (128, 192, 256), (128, 256, 256),
    (160, 64, 256), (160, 128, 256), (160, 192, 256), (160, 256, 256), (192, 128, 256), (192, 192, 256),
    (192, 256, 256), (224, 128, 256), (224, 192, 256), (224, 256, 256), (256, 128, 256), (256, 192, 256),
    (256, 256, 256),
    (32, 32, 768), (32, 32, 1024), (256, 256, 512), (256, 256, 768), (256, 256, 1024),   # the two Pipeline_* loops (:383-403)
]


@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_reference_gtest_problem_list(pk, kind, is_bf16):
    """Same bound as the reference's gtest (max(1e-2, 1 %), :36,53), on its whole problem list, every kernel."""
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    ran = 0
    for (m, n, k) in REFERENCE_GTEST_PROBLEMS:
        a, q, s, gs = random_problem(kind, m, n, k, 31 * m + 7 * n + k, is_bf16)
        ref = oracle_ref(kind, a, is_bf16, q, s, gs)
        sum_abs = oracle_sum_abs(kind, a, is_bf16, q, s, gs)
        for sid in [-1] + list(pk.ops.get_fp4_solutions(h, m, n, k)):
            check_gemm(run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k, sid), ref, is_bf16, sum_abs)
            ran += 1
    assert ran >= 3 * len(REFERENCE_GTEST_PROBLEMS)


def test_unknown_solution_and_bad_shapes_raise(pk):
    a, q, s, gs = random_problem("nv", 1, 64, 256, 5, True)
    with pytest.raises(RuntimeError, match="No kernel implementation for solution_id=4660"):
        run_case(pk, "nv", a, True, q, s, gs, 1, 64, 256, 0x1234)
    z = pk.mul_nvfp4_a16(torch.zeros((0, 256), dtype=torch.bfloat16, device=DEV),
                         torch.zeros((4, 512), dtype=torch.int32, device=DEV),
                         torch.zeros((64, 16), dtype=torch.float8_e4m3fn, device=DEV),
                         torch.ones(1, device=DEV), 0, 64, 256, -1)
    assert z.shape == (0, 64)                                    # gemm_fp4_fp16_grid.cc:42-44


@pytest.mark.parametrize("kind,is_bf16,m,n,k", [("nv", True, 5, 96, 1024), ("mx", True, 33, 64, 512), ("nv", False, 1, 128, 2048)])
def test_cxx_api_end_to_end(pk, tmp_path, kind, is_bf16, m, n, k):
    """A C++ program written against the reference's namespace API (examples/cxx_gemm.cc, include/causalflow/petit/gemm.h)
    repacks and multiplies on the GPU; its output must match the oracle like the Python path does."""
    import struct
    import subprocess
    from petit_kernel import _lib
    a, q, s, gs = random_problem(kind, m, n, k, 2024 + m + n + k, is_bf16)
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        f.write(struct.pack("<5If", 0 if kind == "nv" else 1, int(is_bf16), m, n, k, gs))
        f.write(np.ascontiguousarray(a).tobytes())
        f.write(np.ascontiguousarray(q).tobytes())
        f.write(np.ascontiguousarray(s).tobytes())
    exe = tmp_path / "cxx_gemm"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(ROOT / "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    str(ROOT / "examples/cxx_gemm.cc"), str(_lib.LIB_PATH), f"-Wl,-rpath,{_lib.LIB_PATH.parent}",
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(prob), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    c_bits = np.frombuffer(out.read_bytes(), dtype=np.uint16).reshape(m, n)
    check_gemm(c_bits, oracle_ref(kind, a, is_bf16, q, s, gs), is_bf16, oracle_sum_abs(kind, a, is_bf16, q, s, gs))


def test_hip_graph_capture_and_replay(pk):
    """No entry point synchronises the host or allocates behind the caller's back (SURVEY.md section 8b "Threading /
    streams"): repack + GEMM (plain, fused, native two-launch path) are captured into one HIP graph, the inputs are
    then changed in place, and a replay must produce the new problem's result."""
    m, n, k = 4, 128, 1024
    a1, q1, s1, gs1 = random_problem("mx", m, n, k, 1, True)
    a2, q2, s2, gs2 = random_problem("mx", m, n, k, 2, True)
    a = from_bits(a1, torch.bfloat16).to(DEV)
    q = torch.from_numpy(q1).to(DEV)
    sc = torch.from_numpy(s1).to(DEV)
    gsd = torch.tensor([gs1], dtype=torch.float32, device=DEV)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.mxfloat4_e2m1
    pk.ops.enable_native_fp4(True)
    ws = torch.empty(pk.ops.native_workspace_bytes(m, k), dtype=torch.uint8, device=DEV)
    pk.ops.set_workspace(ws)
    try:
        native = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 32) & 7 == 2][0]
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            def run():
                b = pk.repack_mxfp4(q.view(torch.int32), n, k)
                sp = pk.process_mxfp4_scales(sc, n, k)
                return (pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, -1),
                        pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, -1, activation="silu_mul"),
                        pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, native))
            run()                                   # warm-up outside capture (module load)
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                outs = run()
            a.copy_(from_bits(a2, torch.bfloat16))
            q.copy_(torch.from_numpy(q2))
            sc.copy_(torch.from_numpy(s2))
            gsd.fill_(gs2)
            g.replay()
            stream.synchronize()
        ref = oracle_ref("mx", a2, True, q2, s2, gs2)
        sum_abs = oracle_sum_abs("mx", a2, True, q2, s2, gs2)
        check_gemm(bits(outs[0]), ref, True, sum_abs)
        y = ref.astype(np.float64)
        with np.errstate(over="ignore"):
            act = y[:, : n // 2] / (1.0 + np.exp(-y[:, : n // 2])) * y[:, n // 2:]
        cf = to_f32(bits(outs[1]), True).astype(np.float64)
        fin = np.isfinite(act) & (np.abs(act) < 1e30)
        assert (np.abs(cf - act)[fin] <= np.maximum(1e-2, 2e-2 * np.abs(act))[fin]).all()
        cn = to_f32(bits(outs[2]), True).astype(np.float64)
        assert (np.abs(cn - ref) <= 2e-2 * sum_abs + 1e-2).all()
    finally:
        pk.ops.set_workspace(None)
        pk.ops.enable_native_fp4(False)


def test_concurrent_host_threads_and_streams(pk):
    """Stateless after static init (gemm_fp4_fp16_grid.cc:15-18,31-33 in the reference): four host threads, each on its
    own stream with its own problem, hammer the library concurrently; every result must be its own problem's."""
    import threading
    probs = []
    for i, (m, n, k, kind, is_bf16) in enumerate([(1, 256, 2048, "nv", True), (9, 96, 1024, "mx", True),
                                                   (40, 64, 3072, "nv", False), (130, 128, 1024, "nv", True)]):
        a, q, s, gs = random_problem(kind, m, n, k, 900 + i, is_bf16)
        probs.append((m, n, k, kind, is_bf16, a, q, s, gs, oracle_ref(kind, a, is_bf16, q, s, gs),
                      oracle_sum_abs(kind, a, is_bf16, q, s, gs)))
    errors = []

    def worker(p):
        try:
            m, n, k, kind, is_bf16, a, q, s, gs, ref, sum_abs = p
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(20):
                    check_gemm(run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k), ref, is_bf16, sum_abs)
        except Exception as exc:  # noqa: BLE001
            errors.append(repr(exc))

    threads = [threading.Thread(target=worker, args=(p,)) for p in probs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_two_streams_concurrent_split_k(pk):
    """Two GEMMs that need scratch memory (cross-workgroup K split: stream kernel, tiled kernel) enqueued concurrently on
    two streams of one device from two host threads: the Python layer hands each CALL its own workspace (per-call
    scratch through petit_gemm_*_ws), so nothing can overwrite another call's slabs (round-1 ADVICE: one global
    workspace per device was a silent race)."""
    import threading
    specs = [("nv", True, 24, 512, 8192, 0), ("nv", True, 160, 256, 8192, 8), ("mx", True, 48, 256, 4096, 0), ("mx", True, 130, 128, 4096, 8)]
    probs = []
    for i, (kind, is_bf16, m, n, k, want_kind) in enumerate(specs):
        a, q, s, gs = random_problem(kind, m, n, k, 7000 + i, is_bf16)
        h = pk.PetitSolutionHints()
        h.a_type = h.c_type = torch.bfloat16
        h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
        sid = next(x for x in pk.ops.get_fp4_solutions(h, m, n, k) if (x >> 48) & 0xF == want_kind)
        sid = (sid & ~(0xF << 60)) | (2 << 60)
        assert pk.ops.workspace_bytes(h, m, n, k, sid) == 2 * m * n * 4
        probs.append((kind, is_bf16, m, n, k, sid, a, q, s, gs, oracle_ref(kind, a, is_bf16, q, s, gs),
                      oracle_sum_abs(kind, a, is_bf16, q, s, gs)))
    errors = []

    def worker(p):
        try:
            kind, is_bf16, m, n, k, sid, a, q, s, gs, ref, sum_abs = p
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(25):
                    check_gemm(run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k, sid), ref, is_bf16, sum_abs)
        except Exception as exc:  # noqa: BLE001
            errors.append(repr(exc))

    threads = [threading.Thread(target=worker, args=(p,)) for p in probs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_registered_workspace_serves_one_stream(pk):
    """The legacy per-device workspace (petit_set_workspace) binds to the first stream that uses it: an explicit
    scratch-needing id from another stream is refused loudly instead of racing; AUTO falls back to a kernel without
    scratch; re-registering rebinds."""
    from petit_kernel import _lib
    import ctypes as C
    m, n, k = 24, 256, 4096
    a, q, s, gs = random_problem("nv", m, n, k, 8100, True)
    ref = oracle_ref("nv", a, True, q, s, gs)
    ad = from_bits(a, torch.bfloat16).to(DEV)
    b = pk.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    c = torch.empty((m, n), dtype=torch.bfloat16, device=DEV)
    hints = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1
    sid = next(x for x in pk.ops.get_fp4_solutions(h, m, n, k) if (x >> 48) & 0xF == 0)
    sid = (sid & ~(0xF << 60)) | (2 << 60)
    ws = torch.empty(2 * m * n, dtype=torch.float32, device=DEV)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def call(stream, solution):
        rc = _lib.lib.petit_gemm_fp4_fp16_grid(c.data_ptr(), ad.data_ptr(), b.data_ptr(), sp.data_ptr(), gsd.data_ptr(), m, n, k,
                                               C.byref(hints), C.c_uint64(solution), C.c_void_p(stream.cuda_stream))
        stream.synchronize()
        return rc

    torch.cuda.synchronize()
    assert call(s1, sid) == _lib.PETIT_ERROR_KERNEL_SHAPE           # nothing registered, no per-call scratch
    pk.ops.set_workspace(ws)
    try:
        assert call(s1, sid) == 0
        check_gemm(bits(c), ref, True)
        assert call(s2, sid) == _lib.PETIT_ERROR_BAD_ARGUMENT       # bound to s1: refused, not raced
        assert call(s1, sid) == 0
        c.zero_()
        assert call(s2, _lib.PETIT_SOLUTION_AUTO) == 0              # AUTO never needs the registered scratch
        check_gemm(bits(c), ref, True)
        pk.ops.set_workspace(ws)                                    # re-register: binds again, to whoever comes first
        assert call(s2, sid) == 0
        check_gemm(bits(c), ref, True)
        assert call(s1, sid) == _lib.PETIT_ERROR_BAD_ARGUMENT
    finally:
        pk.ops.set_workspace(None)


@pytest.mark.parametrize("is_bf16", [True, False])
def test_nv_typed_solution_ids_work_with_mxfp4(pk, is_bf16):
    """get_fp4_solutions(m, n, k, a_type, c_type) hard-codes b_type = FP4_E2M1 (petit_kernel/__init__.py:63-66), so
    its ids carry the NVFP4 element nibble; the reference's MX entry point rewrites the nibble and dispatches
    (gemm_fp4_fp16_grid.cc:79-95).  Same here: every such id (block-floating-point ones map to their plain staged
    twins) must run mul_mxfp4_a16, or be refused as a kernel-shape error -- never as garbage."""
    m, n, k = 4, 128, 2048
    a, q, s, gs = random_problem("mx", m, n, k, 8200, is_bf16)
    ref = oracle_ref("mx", a, is_bf16, q, s, gs)
    sum_abs = oracle_sum_abs("mx", a, is_bf16, q, s, gs)
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    ids = pk.get_fp4_solutions(m, n, k, dtype, dtype)
    assert ids and all((sid >> 28) & 0xF == 1 for sid in ids)
    ran = 0
    for sid in ids:
        try:
            c = run_case(pk, "mx", a, is_bf16, q, s, gs, m, n, k, sid)
        except RuntimeError as exc:
            assert "No kernel implementation" in str(exc)
            continue
        check_gemm(c, ref, is_bf16, sum_abs)
        ran += 1
    assert ran >= len(ids) // 2


def test_compiled_and_ctypes_bindings_agree(pk):
    """The compiled torch.library operator layer (csrc/torch_binding.cpp -> torch.ops.petit_kernel.*, the counterpart of
    the reference's ATen extension lib/pybind/fp4.cc) and the ctypes layer are two shims over one C ABI: every op must
    return bit-identical tensors through both, including the fused epilogues and a kernel that needs per-call scratch."""
    from petit_kernel import compiled, ops
    assert compiled.available(), compiled.why_unavailable()
    assert pk._impl is compiled
    for kind, is_bf16, m, n, k in [("nv", True, 3, 96, 1024), ("mx", True, 17, 64, 2048), ("nv", False, 130, 128, 1024), ("mx", False, 5, 64, 512)]:
        dtype = torch.bfloat16 if is_bf16 else torch.float16
        a, q, s, gs = random_problem(kind, m, n, k, 9100 + m, is_bf16)
        ad, qd = from_bits(a, dtype).to(DEV), torch.from_numpy(q).to(DEV).view(torch.int32)
        gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
        bias = torch.randn(n, device=DEV).to(dtype)
        b1, b2 = compiled.repack_nvfp4(qd, n, k), ops.repack_nvfp4(qd, n, k)
        assert torch.equal(b1, b2)
        if kind == "nv":
            sd = torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn)
            s1, s2 = compiled.process_nvfp4_scales(sd, n, k), ops.process_nvfp4_scales(sd, n, k)
            mul1, mul2 = compiled.mul_nvfp4_a16, ops.mul_nvfp4_a16
        else:
            sd = torch.from_numpy(s).to(DEV)
            s1, s2 = compiled.process_mxfp4_scales(sd, n, k), ops.process_mxfp4_scales(sd, n, k)
            mul1, mul2 = compiled.mul_mxfp4_a16, ops.mul_mxfp4_a16
        assert torch.equal(s1.view(torch.uint8), s2.view(torch.uint8))
        h = pk.PetitSolutionHints()
        h.a_type = h.c_type = dtype
        h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
        split = next(x for x in pk.ops.get_fp4_solutions(h, m, n, k) if (x >> 48) & 0xF == 0)
        split = (split & ~(0xF << 60)) | (2 << 60)
        for sid, kw in [(-1, {}), (-1, {"bias": bias}), (-1, {"activation": "silu_mul"}), (split, {})]:
            c1, c2 = mul1(ad, b1, s1, gsd, m, n, k, sid, **kw), mul2(ad, b1, s1, gsd, m, n, k, sid, **kw)
            assert c1.shape == c2.shape and torch.equal(c1.view(torch.int16), c2.view(torch.int16)), (kind, sid, kw)
        check_gemm(bits(mul1(ad, b1, s1, gsd, m, n, k, -1)), oracle_ref(kind, a, is_bf16, q, s, gs), is_bf16,
                   oracle_sum_abs(kind, a, is_bf16, q, s, gs))
        for neg in (-2, -3, -7):   # any negative id is the library default on the reference's entry points (fp4.cc:189,240), through both layers
            assert torch.equal(mul1(ad, b1, s1, gsd, m, n, k, neg).view(torch.int16), mul1(ad, b1, s1, gsd, m, n, k, -1).view(torch.int16))
            assert torch.equal(mul2(ad, b1, s1, gsd, m, n, k, neg).view(torch.int16), mul2(ad, b1, s1, gsd, m, n, k, -1).view(torch.int16))


def test_compiled_ops_trace_without_graph_break(pk):
    """torch.compile(fullgraph=True) through the compiled operator layer: the Meta kernels let dynamo trace
    torch.ops.petit_kernel.mul_nvfp4_a16 as one opaque call (backend "eager": no code generator involved), and the traced
    function returns what the eager call returns."""
    from petit_kernel import compiled
    assert compiled.available(), compiled.why_unavailable()
    m, n, k = 7, 128, 1024
    a, q, s, gs = random_problem("nv", m, n, k, 4711, True)
    ad, qd = from_bits(a, torch.bfloat16).to(DEV), torch.from_numpy(q).to(DEV).view(torch.int32)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    b = compiled.repack_nvfp4(qd, n, k)
    sp = compiled.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)

    def layer(x):
        return torch.ops.petit_kernel.mul_nvfp4_a16(x * 1.0, b, sp, gsd, m, n, k, -1) + 1.0

    try:
        traced = torch.compile(layer, backend="eager", fullgraph=True)
        out = traced(ad)
    except Exception as exc:  # noqa: BLE001 -- dynamo itself unavailable on this build
        if "petit_kernel" in str(exc):
            raise
        pytest.skip(f"torch.compile unavailable here: {type(exc).__name__}")
    assert torch.equal(out.view(torch.int16), layer(ad).view(torch.int16))


def test_offline_repack_matches_device(pk):
    """petit_kernel.offline (CPU, checkpoint-side tooling) == the device repack, bit for bit, and the GEMM
    accepts the CPU-packed tensors."""
    m, n, k = 3, 96, 1024
    a, q, s, gs = random_problem("nv", m, n, k, 99, True)
    qd, sd = torch.from_numpy(q), torch.from_numpy(s).view(torch.float8_e4m3fn)
    b_cpu = pk.offline.repack_nvfp4_cpu(qd.view(torch.int32), n, k)
    s_cpu = pk.offline.process_nvfp4_scales_cpu(sd, n, k)
    b_dev = pk.repack_nvfp4(qd.to(DEV).view(torch.int32), n, k)
    s_dev = pk.process_nvfp4_scales(sd.to(DEV), n, k)
    assert torch.equal(b_cpu, b_dev.cpu()) and torch.equal(s_cpu.view(torch.uint8), s_dev.cpu().view(torch.uint8))
    mx = np.random.default_rng(5).integers(100, 150, (n, k // 32), dtype=np.uint8)
    assert torch.equal(pk.offline.process_mxfp4_scales_cpu(torch.from_numpy(mx), n, k),
                       pk.process_mxfp4_scales(torch.from_numpy(mx).to(DEV), n, k).cpu())
    c = pk.mul_nvfp4_a16(from_bits(a, torch.bfloat16).to(DEV), b_cpu.to(DEV), s_cpu.to(DEV),
                         torch.tensor([gs], dtype=torch.float32, device=DEV), m, n, k, -1)
    check_gemm(bits(c), oracle_ref("nv", a, True, q, s, gs), True)


@pytest.mark.parametrize("m,n,k,splitk", [(1, 256, 2048, 1), (16, 96, 1024, 1), (40, 64, 3072, 1), (130, 128, 1024, 1), (3, 64, 4096, 2)])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True)])
def test_fused_bias_epilogue(pk, kind, is_bf16, m, n, k, splitk):
    """c = round16(acc * gs + bias[n]) (petit_epilogue): every kernel kind, one rounding; without a bias the
    _ex entry point is bit-identical to the plain call."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a, q, s, gs = random_problem(kind, m, n, k, 4321 + m + n + k, is_bf16)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(n)).mul(4.0).to(dtype)
    ref = oracle_ref(kind, a, is_bf16, q, s, gs).astype(np.float64) + bias.float().numpy().astype(np.float64)[None, :]
    ad, qd = from_bits(a, dtype).to(DEV), torch.from_numpy(q).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    if kind == "nv":
        b, sp = pk.repack_nvfp4(qd.view(torch.int32), n, k), pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        mul = pk.mul_nvfp4_a16
    else:
        b, sp = pk.repack_mxfp4(qd.view(torch.int32), n, k), pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        mul = pk.mul_mxfp4_a16
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = dtype
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    sols = pk.ops.get_fp4_solutions(h, m, n, k)
    ws = None
    if splitk > 1:
        ws = torch.empty(splitk * m * n, dtype=torch.float32, device=DEV)
        pk.ops.set_workspace(ws)
        sols = [(sid & ~(0xF << 60)) | (splitk << 60) for sid in sols if (sid >> 48) & 0xF not in (8, 9, 12)][:6]
    try:
        sum_abs = oracle_sum_abs(kind, a, is_bf16, q, s, gs)
        for sid in [-1] + list(sols):
            c = mul(ad, b, sp, gsd, m, n, k, sid, bias=bias.to(DEV))
            check_gemm(bits(c), ref, is_bf16, sum_abs)
        plain = mul(ad, b, sp, gsd, m, n, k, -1)
        zero = mul(ad, b, sp, gsd, m, n, k, -1, bias=torch.zeros(n, dtype=dtype, device=DEV))
        assert torch.equal(plain.view(torch.int16), zero.view(torch.int16))
    finally:
        if ws is not None:
            pk.ops.set_workspace(None)


@pytest.mark.parametrize("m,n,k", [(1, 256, 2048), (7, 96, 1024), (16, 64, 1024), (40, 128, 3072), (130, 256, 1024), (300, 544, 512)])
@pytest.mark.parametrize("kind,is_bf16,with_bias", [("nv", True, False), ("nv", True, True), ("nv", False, True), ("mx", True, False), ("mx", False, True)])
def test_fused_silu_mul_epilogue(pk, kind, is_bf16, with_bias, m, n, k):
    """activation="silu_mul": c[m, j] = silu(y[m, j]) * y[m, j + n/2] with y = acc * gs (+ bias), one rounding.  Every
    enumerated kernel that can serve it (even n-tiles per wave), the default pick, and the refusal of the others."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a, q, s, gs = random_problem(kind, m, n, k, 555 + m + n + k, is_bf16, mx_band=(122, 130))
    y = oracle_ref(kind, a, is_bf16, q, s, gs).astype(np.float64) * 0.05          # keep silu in its curved range
    gs *= 0.05
    bias = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.5).to(dtype) if with_bias else None
    if bias is not None:
        y = y + bias.float().numpy().astype(np.float64)[None, :]
    gate, up = y[:, : n // 2], y[:, n // 2:]
    ref = gate / (1.0 + np.exp(-gate)) * up
    ad, qd = from_bits(a, dtype).to(DEV), torch.from_numpy(q).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    if kind == "nv":
        b, sp = pk.repack_nvfp4(qd.view(torch.int32), n, k), pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        mul = pk.mul_nvfp4_a16
    else:
        b, sp = pk.repack_mxfp4(qd.view(torch.int32), n, k), pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        mul = pk.mul_mxfp4_a16
    bd = bias.to(DEV) if bias is not None else None
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = dtype
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    served = refused = 0
    for sid in [-1] + list(pk.ops.get_fp4_solutions(h, m, n, k)):
        nt = (sid >> 52) & 0xF if sid >= 0 else 2
        shared = sid >= 0 and (sid >> 48) & 0xF == 12 and (sid >> 36) & 0xF == 5   # gemm_shared.hpp: plain / bias epilogue only
        if nt % 2 or shared:
            with pytest.raises(RuntimeError, match="No kernel implementation"):
                mul(ad, b, sp, gsd, m, n, k, sid, bias=bd, activation="silu_mul")
            refused += 1
            continue
        c = mul(ad, b, sp, gsd, m, n, k, sid, bias=bd, activation="silu_mul")
        assert c.shape == (m, n // 2) and c.dtype == dtype
        cf = to_f32(bits(c), is_bf16).astype(np.float64)
        # two rounded-once f32 factors multiplied: twice the relative bound of the plain GEMM, same absolute floor
        err = np.abs(cf - ref)
        assert (err <= np.maximum(1e-2, 2e-2 * np.abs(ref))).all(), f"sid {sid:#x}: max err {err.max()}"
        served += 1
    assert served >= 2
    # with a cross-workgroup K split the reduce pass applies SiLU-mul over plain slabs: every kernel serves it then, the ones above that
    # refuse it unsplit included (odd n-tiles per wave, the LDS-shared kernel)
    split_served = 0
    for sid in pk.ops.get_fp4_solutions(h, m, n, k):
        ks = ((sid >> 16) & 0x1F) // 2                        # k-tiles per span: a split needs a span per part
        kind_nib = (sid >> 48) & 0xF
        if kind_nib in (9, 13) or k // (128 * ks) < 2:        # (the native class has its own accuracy bound: test_native_*)
            continue
        if kind_nib == 0 and (sid >> 36) & 0xF == 2 and k // (128 * ks) < 2 * ((sid >> 44) & 0xF):
            continue                                          # (gemm_batch.hpp splits K over its WK in-workgroup parts first: a slice needs WK spans)
        sid2 = (sid & ~(0xF << 60)) | (2 << 60)
        try:
            plain = mul(ad, b, sp, gsd, m, n, k, sid2)        # does this kernel take a 2-way split of this K at all?
        except RuntimeError:
            continue
        del plain
        c = mul(ad, b, sp, gsd, m, n, k, sid2, bias=bd, activation="silu_mul")
        assert c.shape == (m, n // 2) and c.dtype == dtype
        err = np.abs(to_f32(bits(c), is_bf16).astype(np.float64) - ref)
        assert (err <= np.maximum(1e-2, 2e-2 * np.abs(ref))).all(), f"sid {sid2:#x}: max err {err.max()}"
        split_served += 1
    assert split_served >= 2 or k < 2048


@pytest.mark.parametrize("m", [16, 40, 130])
@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("k", [256, 512, 1024])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("mx", False)])
def test_silu_mul_with_a_k_split_that_collapses(pk, kind, is_bf16, m, n, k):
    """K of one span (256 / 512 / 1024 at span sizes 2 / 4 / 8) with a split nibble of 2: the launch has one K slice and no reduce pass, so SiLU-mul is
    the kernel's own epilogue's job.  Every enumerated tiled, wide, LDS-shared and batched-decode kernel: bit-identical to its unsplit launch when its
    epilogue can apply the activation, refused when it cannot (odd n-tiles per wave, the LDS-shared kernel) -- never C unwritten or plain.  The same for
    one 32x32x64 native kernel per activation format (MXFP4 weights), and the default pick stays within the SiLU-mul bound against the oracle."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    a, q, s, gs = random_problem(kind, m, n, k, 777 + m + n + k, is_bf16, mx_band=(122, 130))
    y = oracle_ref(kind, a, is_bf16, q, s, gs).astype(np.float64) * 0.05          # keep silu in its curved range
    gs *= 0.05
    bias = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.5).to(dtype)
    y = y + bias.float().numpy().astype(np.float64)[None, :]
    gate, up = y[:, : n // 2], y[:, n // 2:]
    ref = gate / (1.0 + np.exp(-gate)) * up
    ad, qd, bd = from_bits(a, dtype).to(DEV), torch.from_numpy(q).to(DEV), bias.to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    if kind == "nv":
        b, sp = pk.repack_nvfp4(qd.view(torch.int32), n, k), pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        mul = pk.mul_nvfp4_a16
    else:
        b, sp = pk.repack_mxfp4(qd.view(torch.int32), n, k), pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        mul = pk.mul_mxfp4_a16
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = dtype
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1

    def split2_is_unsplit_or_refused(sid):
        sid2 = (sid & ~(0xF << 60)) | (2 << 60)
        shared = (sid >> 48) & 0xF == 12 and (sid >> 36) & 0xF == 5
        if ((sid >> 52) & 0xF) % 2 or shared:
            with pytest.raises(RuntimeError, match="No kernel implementation"):
                mul(ad, b, sp, gsd, m, n, k, sid2, bias=bd, activation="silu_mul")
            return False
        c1 = mul(ad, b, sp, gsd, m, n, k, sid, bias=bd, activation="silu_mul")
        c2 = mul(ad, b, sp, gsd, m, n, k, sid2, bias=bd, activation="silu_mul")
        assert c2.shape == (m, n // 2) and torch.equal(c1.view(torch.int16), c2.view(torch.int16)), f"sid {sid2:#x}"
        return True

    kinds = set()
    for sid in pk.ops.get_fp4_solutions(h, m, n, k):
        kind_nib, wm = (sid >> 48) & 0xF, (sid >> 36) & 0xF
        assert k // (128 * (((sid >> 16) & 0x1F) // 2)) == 1          # one span: nothing to split
        if kind_nib == 8 or kind_nib == 12 or (kind_nib == 0 and wm == 2):
            kinds.add((kind_nib, wm == 5, split2_is_unsplit_or_refused(sid)))
    assert any(served for _, _, served in kinds), kinds
    if kind == "mx":
        pk.ops.enable_native_fp4(True)
        try:
            native = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF == 13]
            for code in (2, 4, 6):                                    # activations quantised to MXFP8 / MXFP6 / MXFP4
                assert split2_is_unsplit_or_refused(next(sid for sid in native if (sid >> 32) & 7 == code))
        finally:
            pk.ops.enable_native_fp4(False)
    c = mul(ad, b, sp, gsd, m, n, k, -1, bias=bd, activation="silu_mul")
    err = np.abs(to_f32(bits(c), is_bf16).astype(np.float64) - ref)
    assert (err <= np.maximum(1e-2, 2e-2 * np.abs(ref))).all(), f"default pick: max err {err.max()}"


# --- adversarial activations: the kernels must not depend on the activations' dynamic range ---------------

SPAN = 1024   # k per span at KS = 8: the block-floating-point unit of the Bf16Bfp kernels (csrc/gemm_stream.hpp)


def adversarial_activations(m, k, q, is_bf16, seed, profile):
    """Rows x spans of hostile data.  Span types cycle so that every wave of every K split meets several
    (profile 0: types 0 2 3 4 6, whose contributions to the result are all O(1) so that what an inexact conversion of a
    type-2 span loses is visible at the 1 % bound; profile 1: types 1 and 5 as well, results dominated by huge terms):
      0 N(0,1)                         1 N(0,1) * 2^U[-17,17]: 35 binades inside one span
      2 O(1) values + one huge outlier at a column whose weights are ALL ZERO (the small values carry the
        result, an fp16 block-floating-point span would truncate them)     3 all zero (incl. -0.0)
      4 subnormals of the activation type next to one normal value          5 tiny values + an outlier with weight
      6 N(0,1) (exact BFP span AFTER hostile ones: the switch is one-way per wave)
    Returns (a_bits, q) -- q is edited in place so that type-2 outlier columns hold weight code 0 / 8 (+-0)."""
    rng = np.random.default_rng(seed)
    big = 2.0 ** 36 if is_bf16 else 32768.0
    a = np.zeros((m, k), dtype=np.float32)
    raw_sub = np.zeros((m, k), dtype=bool)
    sub_bits = np.zeros((m, k), dtype=np.uint16)
    for row in range(m):
        for sp in range(k // SPAN):
            sl = slice(sp * SPAN, (sp + 1) * SPAN)
            t = ((0, 2, 3, 4, 6, 2, 0, 2) if profile == 0 else (1, 5, 0, 2, 1, 4, 6, 5))[(sp + 3 * row) % 8]
            x = rng.standard_normal(SPAN).astype(np.float32)
            if t == 1:
                x = x * np.exp2(rng.integers(-17, 18, SPAN) if is_bf16 else rng.integers(-10, 4, SPAN)).astype(np.float32)
            elif t == 2:
                col = int(rng.integers(0, SPAN))
                x[col] = big * (1 if rng.random() < 0.5 else -1)
                q[:, (sp * SPAN + col) // 2] &= (0x80 if col % 2 else 0x08) | (0x0F if col % 2 else 0xF0)  # magnitude bits -> 0
            elif t == 3:
                x[:] = 0.0
                x[::3] = -0.0
            elif t == 4:
                x[:] = 0.0
                raw_sub[row, sl] = True
                sub_bits[row, sl] = rng.integers(1, 0x80 if is_bf16 else 0x400, SPAN).astype(np.uint16) | \
                    (rng.integers(0, 2, SPAN).astype(np.uint16) << 15)
                raw_sub[row, sp * SPAN + 5] = False
                x[5] = 1.5
            elif t == 5:
                x = x * np.float32(1e-6)
                x[int(rng.integers(0, SPAN))] = big
            a[row, sl] = x
    a_bits = O.f32_to_bf16_bits(a) if is_bf16 else a.astype(np.float16).view(np.uint16)
    a_bits = np.where(raw_sub, sub_bits, a_bits).astype(np.uint16)
    return a_bits, q


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 4, 7])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_adversarial_activations_every_solution(pk, kind, is_bf16, m, profile):
    """Outliers, 35-binade spans, subnormals, zero spans: every enumerated kernel (the block-floating-point
    Bf16Bfp ones in particular: they must detect the spans they cannot convert exactly and run those through the
    bf16 pipeline) against the oracle at the usual 1e-2 bound.  K = 16 spans, so waves own several spans each."""
    n, k = 64, 16 * SPAN
    _, q, s, gs = random_problem(kind, m, n, k, 31337 + m, is_bf16, mx_band=(124, 130))
    a, q = adversarial_activations(m, k, q, is_bf16, 4000 + m, profile)
    ref = oracle_ref(kind, a, is_bf16, q, s, gs)
    sum_abs = oracle_sum_abs(kind, a, is_bf16, q, s, gs)
    coef = 1e-5
    if kind == "nv" and profile == 1:
        # outputs whose 2^36-sized terms cancel to 1e-6 of their size: what remains is the f32 accumulation floor of
        # ANY implementation that sums in f32 (the reference's MFMA accumulators included): a few ulp of the largest
        # partial sum (measured: 7e4 on terms of 1e12 = 0.6 ulp).  2^-20 of sum|a||w|, 10x tighter than the MX allowance.
        dq = np.abs(O.dequant_nvfp4(q, s))
        sum_abs, coef = (np.abs(to_f32(a, is_bf16)) @ dq.T) * gs, 2.0 ** -20
    assert np.isfinite(ref).all()
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    sols = pk.ops.get_fp4_solutions(h, m, n, k)
    if kind == "nv" and is_bf16 and m <= 4:
        assert any((sid >> 48) & 0xF in (5, 6, 7) for sid in sols), "the block-floating-point kernels must be in the list"
    if kind == "nv" and m <= 4:
        assert any((sid >> 48) & 0xF in (4, 14, 15) for sid in sols), "the scale-after-MFMA decode kernels must be in the list"
    for sid in [-1] + list(sols):
        c = run_case(pk, kind, a, is_bf16, q, s, gs, m, n, k, sid)
        try:
            check_gemm(c, ref, is_bf16, sum_abs, coef)
        except AssertionError as exc:
            raise AssertionError(f"solution {sid:#x}: {exc}") from None


@pytest.mark.parametrize("m", [1, 4])
def test_nonfinite_activations(pk, m):
    """+-inf / NaN in the activations propagate like IEEE arithmetic does in the oracle: NaN where the oracle has NaN
    (inf x zero weight, NaN x anything), the same signed infinity elsewhere, finite outputs untouched -- every
    bf16 x NVFP4 kernel, BFP included (an inf makes the span's range check fail or scales to inf, both correct)."""
    n, k = 64, 4 * SPAN
    a, q, s, gs = random_problem("nv", m, n, k, 777 + m, True)
    a = a.copy()
    a[0, 100] = 0x7F80                      # +inf in span 0
    a[m - 1, 2 * SPAN + 7] = 0xFF80         # -inf in span 2
    if m > 1:
        a[1, 3 * SPAN + 9] = 0x7FC0         # NaN in row 1
    q[::2, 50] &= 0x80                       # column 100 = low nibble of byte 50: zero weight for even n -> inf * 0 = NaN there
    with np.errstate(all="ignore"):
        ref = oracle_ref("nv", a, True, q, s, gs)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1
    for sid in [-1] + list(pk.ops.get_fp4_solutions(h, m, n, k)):
        got = to_f32(run_case(pk, "nv", a, True, q, s, gs, m, n, k, sid), True)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{sid:#x}"
        inf = np.isinf(ref)
        assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(ref[inf])), f"{sid:#x}"
        fin = np.isfinite(ref)
        if fin.any():
            assert (np.abs(got - ref)[fin] <= np.maximum(1e-2, 1e-2 * np.abs(ref[fin]))).all(), f"{sid:#x}"


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("is_bf16", [True, False])
def test_decode_kernels_extreme_range(pk, m, is_bf16):
    """The scale-after-MFMA decode kernels (csrc/gemm_decode.hpp, kinds 4 / 14 / 15) sum a * w4 per scale group BEFORE the
    group scale is applied.  Activations near the top of the type's range times |w4| = 6 x 16 terms must not overflow
    f32 where the pre-scaled form (e4m3 scales of 2^-9 .. 2^-7 here) stays finite: a handful of huge activations per row, random
    signs, small scales and global scale.  Every decode kernel and the default choice against the oracle."""
    n, k = 64, 8 * SPAN
    rng = np.random.default_rng(99 + m)
    a = rng.standard_normal((m, k)).astype(np.float32)
    top = 2.0 ** 126 if is_bf16 else 32768.0
    for row in range(m):
        cols = rng.choice(k, 8, replace=False)
        a[row, cols] = top * rng.choice([-1.0, 1.0], 8) * rng.uniform(0.5, 1.0, 8)
        # a whole scale group of same-sign near-maximum values: 16 x 6 x 2^126 > f32 max without the kernel's 2^-7
        g0 = 16 * int(rng.integers(0, k // 16))
        a[row, g0:g0 + 16] = top * 0.9
    a_bits = O.f32_to_bf16_bits(a) if is_bf16 else a.astype(np.float16).view(np.uint16)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    sf = np.exp2(rng.integers(-9, -6, (n, k // 16))).astype(np.float32) * rng.choice([1.0, 1.25, 1.75], (n, k // 16)).astype(np.float32)
    s = torch.from_numpy(sf).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    gs = 2.0 ** -12 if is_bf16 else 2.0 ** -6
    with np.errstate(over="ignore"):
        ref = oracle_ref("nv", a_bits, is_bf16, q, s, gs)
    assert np.isfinite(ref).all() and np.abs(ref).max() > (1e30 if is_bf16 else 1.0)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.float4_e2m1
    decode = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF in (4, 14, 15)]
    assert decode
    for sid in [-1] + decode:
        got = to_f32(run_case(pk, "nv", a_bits, is_bf16, q, s, gs, m, n, k, sid), is_bf16)
        assert np.isfinite(got).all(), f"{sid:#x}: spurious overflow"
        assert (np.abs(got - ref) <= np.maximum(1e-2, 1e-2 * np.abs(ref))).all(), f"{sid:#x}"


# --- BASELINE.json full sizes: oracle on the whole problem + size-independent properties --

@pytest.mark.parametrize("m", [1, 16])
def test_full_size_8192_vs_oracle(pk, m):
    """configs[1]: M=1 (and 16), N=K=8192, bf16 x nvfp4, checked against the oracle on every
    output (the C oracle does 8192^2 in about a second)."""
    n = k = 8192
    a, q, s, gs = random_problem("nv", m, n, k, 1234, True)
    c = run_case(pk, "nv", a, True, q, s, gs, m, n, k)
    check_gemm(c, oracle_ref("nv", a, True, q, s, gs), True)


@pytest.mark.parametrize("n,k", [(10240, 8192), (8192, 28672)])
def test_llama70b_shapes_properties(pk, n, k):
    """configs[2] shapes (qkv, down): properties that need no reference at this size --
    (1) zero activations give exactly zero; (2) a one-hot activation row reads back one
    dequantised weight column exactly; (3) rows of a batch are independent: row i of an
    M=8 call equals the M=1 call on that row, bit for bit; (4) sampled outputs vs the oracle."""
    rng = np.random.default_rng(n ^ k)
    _, q, s, gs = random_problem("nv", 1, n, k, 99, True)
    qd = torch.from_numpy(q).to(DEV)
    b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
    sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    gsd = torch.tensor([1.0], dtype=torch.float32, device=DEV)
    zero = torch.zeros((4, k), dtype=torch.bfloat16, device=DEV)
    assert torch.count_nonzero(pk.mul_nvfp4_a16(zero, b, sp, gsd, 4, n, k, -1)) == 0
    cols = [0, 1, 31, 32, 127, 128, 1023, 1024, k // 2 + 17, k - 1]
    onehot = torch.zeros((len(cols), k), dtype=torch.bfloat16, device=DEV)
    for i, c_ in enumerate(cols):
        onehot[i, c_] = 1.0
    got = pk.mul_nvfp4_a16(onehot, b, sp, gsd, len(cols), n, k, -1).float().cpu().numpy()
    lut = O.FP4_VALUES
    for i, c_ in enumerate(cols):
        nib = (q[:, c_ // 2] >> (4 * (c_ % 2))) & 15
        want = lut[nib] * O.e4m3_to_f32(s[:, c_ // 16])
        assert np.array_equal(got[i], want)
    a8 = torch.randn((8, k), dtype=torch.bfloat16, device=DEV)
    c8 = pk.mul_nvfp4_a16(a8, b, sp, gsd, 8, n, k, -1)
    # same kernel for both calls: different solutions split K differently and may round the
    # f32 sum differently in the last bit, which is legitimate
    sid = [x for x in pk.get_fp4_solutions(8, n, k, torch.bfloat16, torch.bfloat16) if (x >> 48) & 0xF == 0][0]
    c8s = pk.mul_nvfp4_a16(a8, b, sp, gsd, 8, n, k, sid)
    for i in (0, 5):
        c1 = pk.mul_nvfp4_a16(a8[i:i + 1].contiguous(), b, sp, gsd, 1, n, k, sid)
        assert torch.equal(c1[0], c8s[i])
    rows = rng.integers(0, n, 64)
    dq = O.dequant_nvfp4(q[rows], s[rows])
    _, cf = O.gemm_ref(bits(a8), True, dq, 1.0)
    check_gemm(bits(c8[:, torch.from_numpy(rows).to(DEV)]), cf, True)


LLAMA70B = {"qkv": (10240, 8192), "o": (8192, 8192), "gate_up": (57344, 8192), "down": (8192, 28672)}


class FullSizeProblem:
    """One Llama-3-70B linear at its real size on the device (BASELINE.json configs[2..4]); weights are drawn and
    repacked once per (kind, shape) and reused for every M / dtype / solution of the test."""

    def __init__(self, pk, kind, n, k, seed):
        self.pk, self.kind, self.n, self.k = pk, kind, n, k
        _, self.q, self.s, _ = random_problem(kind, 1, n, k, seed, True)
        qd = torch.from_numpy(self.q).to(DEV)
        if kind == "nv":
            self.b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
            self.sp = pk.process_nvfp4_scales(torch.from_numpy(self.s).to(DEV).view(torch.float8_e4m3fn), n, k)
            self.mul = pk.mul_nvfp4_a16
        else:
            self.b = pk.repack_mxfp4(qd.view(torch.int32), n, k)
            self.sp = pk.process_mxfp4_scales(torch.from_numpy(self.s).to(DEV), n, k)
            self.mul = pk.mul_mxfp4_a16
        del qd
        self.gs = 0.75
        self.gsd = torch.tensor([self.gs], dtype=torch.float32, device=DEV)
        rng = np.random.default_rng(seed + 1)
        # 64 sampled output columns, always including the first and last n-tile (largest buffer offsets)
        self.rows = np.unique(np.concatenate([rng.integers(0, n, 60), [0, 15, n - 16, n - 1]]))
        dq = O.dequant_nvfp4(self.q[self.rows], self.s[self.rows]) if kind == "nv" else O.dequant_mxfp4(self.q[self.rows], self.s[self.rows])
        self.dq = dq
        self._image = None

    @property
    def image(self):
        """NVFP4 weights on the native class: the MFMA-native image (built once, attached to the packed weights), and the sampled rows as the image
        holds them (oracle.nv6_reencode) with the stated per-element re-rounding bound."""
        if self._image is None:
            assert self.kind == "nv"
            self._image = self.pk.nvfp4_native_image(self.b, self.sp, self.n, self.k)
            self.pk.attach_nvfp4_native(self.b, self._image)
            self.dq_native, sb = O.nv6_reencode(self.q[self.rows], self.s[self.rows])
            self.w_rebound = np.maximum(2.0 ** -4 * np.abs(self.dq), np.repeat(np.ldexp(1.0, sb.astype(np.int64) - 127 - 4), 32, axis=1))
            assert (np.abs(self.dq_native - self.dq) <= self.w_rebound).all()
        return self._image

    def __del__(self):
        if getattr(self, "_image", None) is not None:
            self.pk.attach_nvfp4_native(self.b, None)

    def hints(self, is_bf16):
        h = self.pk.PetitSolutionHints()
        h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
        h.b_type = self.pk.DataType.float4_e2m1 if self.kind == "nv" else self.pk.DataType.mxfloat4_e2m1
        return h

    def activations(self, m, is_bf16, seed):
        a = np.random.default_rng(seed).standard_normal((m, self.k), dtype=np.float32)
        return O.f32_to_bf16_bits(a) if is_bf16 else a.astype(np.float16).view(np.uint16)

    def run(self, a_bits, is_bf16, sid=-1):
        dtype = torch.bfloat16 if is_bf16 else torch.float16
        m = a_bits.shape[0]
        # (the native-class sentinels name that class on its own entry point only; the reference's entry points read any negative id as -1)
        sentinel = sid in (self.pk.SOLUTION_AUTO_NATIVE_MXFP8, self.pk.SOLUTION_AUTO_NATIVE_MXFP6, self.pk.SOLUTION_AUTO_NATIVE_MXFP4)
        if self.kind == "nv" and (sentinel or (sid > 0 and (sid >> 48) & 0xF == 13)):
            # NVFP4 weights on the native class: sentinels through the reference's entry point (the image is attached), explicit ids through the class's own
            _ = self.image
            if sentinel:
                c = self.mul(from_bits(a_bits, dtype).to(DEV), self.b, self.sp, self.gsd, m, self.n, self.k, sid)
            else:
                c = self.pk.mul_nvfp4_native(from_bits(a_bits, dtype).to(DEV), self.image, self.gsd, m, self.n, self.k, sid)
            torch.cuda.synchronize()
            return c
        mul = self.pk.mul_mxfp4_native if sentinel else self.mul
        c = mul(from_bits(a_bits, dtype).to(DEV), self.b, self.sp, self.gsd, m, self.n, self.k, sid)
        torch.cuda.synchronize()
        return c

    def check_sampled(self, c, a_bits, is_bf16, tag=""):
        _, cf = O.gemm_ref(a_bits, is_bf16, self.dq, self.gs)
        sum_abs = None
        if self.kind == "mx":
            sum_abs = (np.abs(to_f32(a_bits, is_bf16)) @ np.abs(self.dq).T) * self.gs
        try:
            check_gemm(bits(c[:, torch.from_numpy(self.rows).to(DEV)]), cf, is_bf16, sum_abs)
        except AssertionError as exc:
            raise AssertionError(f"{tag}: {exc}") from None

    def check_properties(self, m, is_bf16, sid=-1):
        """zero in -> zero out; one-hot rows read back exact dequantised weight columns (every output column)."""
        dtype = torch.bfloat16 if is_bf16 else torch.float16
        k, n = self.k, self.n
        zero = torch.zeros((m, k), dtype=dtype, device=DEV)
        assert torch.count_nonzero(self.mul(zero, self.b, self.sp, torch.ones(1, device=DEV), m, n, k, sid)) == 0
        cols = sorted({c_ for c_ in (0, 31, 32, 127, 128, 1023, 1024, k // 2 + 17, k - 1) if c_ < k})[:m]
        onehot = torch.zeros((m, k), dtype=dtype, device=DEV)
        for i, c_ in enumerate(cols):
            onehot[i, c_] = 1.0
        got = self.mul(onehot, self.b, self.sp, torch.ones(1, device=DEV), m, n, k, sid).float().cpu().numpy()
        for i, c_ in enumerate(cols):
            nib = (self.q[:, c_ // 2] >> (4 * (c_ % 2))) & 15
            sc = O.e4m3_to_f32(self.s[:, c_ // 16]) if self.kind == "nv" else O.e8m0_to_f32(self.s[:, c_ // 32])
            assert np.array_equal(got[i], O.FP4_VALUES[nib] * sc), f"one-hot column {c_}"


def test_gate_up_full_size_bf16_nvfp4(pk):
    """configs[2], the widest shape: gate_up 57344 x 8192 at M in {1, 4, 8, 16, 32} through solution_id = -1 (M = 9..32
    takes the 16x256 / 32x256 tiled kernels via the arch table: the largest buffer offsets in the library) and through
    one explicit kernel of each kind that serves that M."""
    n, k = LLAMA70B["gate_up"]
    P = FullSizeProblem(pk, "nv", n, k, 57344)
    for m in (1, 4, 8, 16, 32):
        a = P.activations(m, True, 100 + m)
        P.check_properties(m, True)
        P.check_sampled(P.run(a, True), a, True, f"auto M={m}")
        sols = pk.ops.get_fp4_solutions(P.hints(True), m, n, k)
        by_kind = {}
        for sid in sols:
            by_kind.setdefault((sid >> 48) & 0xF, sid)
        for sid in by_kind.values():
            P.check_sampled(P.run(a, True, sid), a, True, f"M={m} sid={sid:#x}")


@pytest.mark.parametrize("shape", ["qkv", "o", "gate_up", "down"])
def test_llama70b_fp16_mxfp4_full_size(pk, shape):
    """configs[3]: MXFP4 weights (e8m0 block scales) x fp16 activations on every Llama-3-70B linear, M in {1, 16}:
    default pick + one explicit kernel per kind, properties + sampled columns vs the oracle."""
    n, k = LLAMA70B[shape]
    P = FullSizeProblem(pk, "mx", n, k, n + k)
    for m in (1, 16):
        a = P.activations(m, False, 200 + m)
        P.check_properties(m, False)
        P.check_sampled(P.run(a, False), a, False, f"auto M={m}")
        by_kind = {}
        for sid in pk.ops.get_fp4_solutions(P.hints(False), m, n, k):
            by_kind.setdefault((sid >> 48) & 0xF, sid)
        for sid in by_kind.values():
            P.check_sampled(P.run(a, False, sid), a, False, f"M={m} sid={sid:#x}")


def native_exact_bound(a_q: np.ndarray, w: np.ndarray, gs: float, fmt: str) -> np.ndarray:
    """Per-output bound on |kernel - exact| for the native (block-scaled MFMA) kernels, DERIVED from what the instruction does
    (tools/probes/mfma_scale_align.hip, profiles/r05_mfma_scale_align.txt; include/petit_amd.h states it), fmt = "mxfp8" / "mxfp6" / "mxfp4".
    Measured on gfx950, identically for v_mfma_scale_f32_32x32x64 and 16x16x128:
      (1) every activation format: the partial sums of one 32-element block and the incoming accumulator are aligned to the largest of them and each is
          TRUNCATED to a multiple of 2^(E - 24), E = floor(log2(largest)); their sum is then exact.  (A term in ANOTHER block of the same instruction
          survives next to +-big of any size; with FP6 / FP4 activations a block's own sum is exact: 0 units of error over thousands of random blocks.)
          A block therefore costs at most 33 * 2^-24 * max(P_b, T), P_b = the block's largest |a w|, T = sum over blocks of |block sum| (no
          accumulation order or K split has a larger partial sum); the <= 16 cross-wave / cross-slice f32 additions cost 2^-24 * T each.
      (2) FP8 (e4m3) activations only: inside a block the products are first summed in GROUPS of 8 consecutive k, aligned to the group's largest
          product and truncated to 14 bits below it: a pair (6 * 448, 0.5 * small) in one group keeps 14 significant bits of its sum whatever the gap,
          24 when the two sit in different groups (PAIRSUM lines of the probe); unit = 2^(e_a + e_w - 13) <= P_g * 2^-13.  A group of 8 costs at
          most 7 truncations: 7 * 2^-13 * P_g, P_g = the group's largest |a w|.
        bound = gs * [ 2^-24 * (33 * sum_b max(P_b, T) + 16 * T)  +  (fmt == "mxfp8") * 7 * 2^-13 * sum_g P_g ]
    P_b is bounded by max|a| * max|w| over the block; P_g is taken from the products themselves when the problem is small enough to form them, else
    bounded the same way over the group.  a_q [m, K] (the quantised activations, dequantised), w [n, K] (dequantised weights without the global
    scale) -> [m, n]."""
    m, k = a_q.shape
    n = w.shape[0]
    nb = k // 32
    A = np.ascontiguousarray(a_q.astype(np.float32).reshape(m, nb, 32).transpose(1, 0, 2))        # [nb, m, 32]
    W = w.astype(np.float32).reshape(n, nb, 32)
    amax = np.abs(A).max(axis=2)                                                                   # [nb, m]
    out = np.empty((m, n))
    step = max(1, (16 << 20) // max(1, m * nb))                # column chunks: [nb, m, chunk] stays under ~64 MB of f32
    for c0 in range(0, n, step):
        Wc = np.ascontiguousarray(W[c0:c0 + step].transpose(1, 2, 0))                              # [nb, 32, chunk]
        bs = np.matmul(A, Wc)                                   # block sums [nb, m, chunk] (f32: only their magnitude enters the bound; x 1.001 below)
        T = np.abs(bs).sum(axis=0, dtype=np.float64) * 1.001
        pmax = amax[:, :, None] * np.abs(Wc).max(axis=1)[:, None, :]
        mx = np.maximum(pmax, T[None, :, :].astype(np.float32))          # (2^floor(log2 x) <= x: the truncation unit of a block is at most max(P_b, T) 2^-24)
        out[:, c0:c0 + step] = 2.0 ** -24 * (33.0 * mx.sum(axis=0, dtype=np.float64) + 16.0 * T)
    if fmt == "mxfp8":
        ng = k // 8
        a8, w8 = np.abs(a_q.astype(np.float32)).reshape(m, ng, 8), np.abs(w.astype(np.float32)).reshape(n, ng, 8)
        if m * n * k <= 3e8:                                    # the products themselves: max over the group of |a_i w_i|
            grp = np.empty((m, n))
            for r0 in range(0, m, max(1, (1 << 25) // max(1, n * k))):
                r1 = min(m, r0 + max(1, (1 << 25) // max(1, n * k)))
                grp[r0:r1] = (a8[r0:r1, None, :, :] * w8[None, :, :, :]).max(axis=3).sum(axis=2, dtype=np.float64)
        else:                                                   # max|a| * max|w| over the group (an upper bound of it)
            grp = a8.max(axis=2).astype(np.float64) @ w8.max(axis=2).astype(np.float64).T
        out += 7.0 * 2.0 ** -13 * grp
    return abs(gs) * out


def native_p99_guard(err, exact, sum_abs, tag=""):
    """native_exact_bound is a WORST case (every truncation a full unit, every block charged the final magnitude): on cancelling outputs it is
    10-50 x looser than the empirical 4e-5 * sum|a||w| of rounds 3-4, which a kernel that dropped a low-order block contribution could hide under.  So next
    to it: at most 1 % of the outputs may exceed max(one 16-bit rounding's 1e-2 bound, 4e-5 * sum|a||w|) -- the old tolerance as a p99, not as a maximum."""
    over = err > np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), 4e-5 * sum_abs)
    assert over.mean() <= 0.01, f"{tag}: {over.mean():.4f} of the outputs beyond the p99 guard"


def check_native_sampled(P, c, a_bits, act_code, tag):
    """A native-FP4 kernel's output on FullSizeProblem P's sampled columns: (1) exact semantics against the oracle run on the
    CPU-quantised activations (usual 1e-2 bound), (2) the class's stated end-to-end tolerance against the unquantised oracle
    (act_code 2 = MXFP8 activations: 2e-2 * sum|a||w| + 1e-2; 4 = MXFP6 e2m3: the same bound; 6 = MXFP4: 0.12 * sum|a||w| + 1e-2)."""
    cache = P.__dict__.setdefault("_native_refs", {})
    key = (act_code, a_bits.shape, a_bits.tobytes()[:64], int(a_bits.view(np.uint16).sum()))   # (the references depend on the activations only)
    if key not in cache:
        a_f32 = to_f32(a_bits, True)
        a_q = {2: quantize_act_mxfp8, 4: quantize_act_mxfp6, 6: quantize_act_mxfp4}[act_code](a_f32)
        # NVFP4 weights run on their MFMA-native image: exact semantics on the image's values; against the unquantised oracle (the TRUE NVFP4 weights) the
        # class tolerance widens by the stated re-rounding bound of the weights, sum_k |a_k| max(2^-4 |w_k|, 2^(E_k - 4))  (include/petit_amd.h)
        if P.kind == "nv":
            _ = P.image
        dq_run = P.dq_native if P.kind == "nv" else P.dq
        _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq_run, P.gs)
        _, full = O.gemm_ref(a_bits, True, P.dq, P.gs)
        sum_abs = (np.abs(a_f32) @ np.abs(P.dq).T) * P.gs
        if P.kind == "nv":
            sum_abs = sum_abs + (np.abs(a_f32) @ P.w_rebound.T) * P.gs / {2: 2e-2, 4: 2e-2, 6: 0.12}[act_code]   # (enters as coef * sum_abs below)
        cache[key] = (exact, full, sum_abs, native_exact_bound(a_q, dq_run, P.gs, {2: "mxfp8", 4: "mxfp6", 6: "mxfp4"}[act_code]),
                      (np.abs(a_q) @ np.abs(dq_run).T) * P.gs)
    exact, full, sum_abs, derived, sum_abs_q = cache[key]
    got = to_f32(bits(c[:, torch.from_numpy(P.rows).to(DEV)]), True).astype(np.float64)
    err = np.abs(got - exact)
    # (the derived per-output bound replaces rounds 3-4's empirical 1e-5 ... 4e-5 of sum|a||w|: native_exact_bound)
    assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)).all(), f"{tag}: exact-semantics max err {err.max()}"
    native_p99_guard(err, exact, sum_abs_q, tag)
    # ... and much tighter on average (the derived bound is a worst case: every truncation a full unit, all in one direction): one 16-bit rounding
    assert np.median(err / np.maximum(np.abs(exact), 1e-3)) < 2 ** -8, f"{tag}: median relative error {np.median(err / np.maximum(np.abs(exact), 1e-3))}"
    coef = 2e-2 if act_code in (2, 4) else 0.12
    assert (np.abs(got - full) <= coef * sum_abs + 1e-2).all(), f"{tag}: class tolerance"


@pytest.mark.parametrize("shape", ["o", "qkv", "gate_up", "down"])
@pytest.mark.parametrize("kind", ["nv", "mx"])
def test_m512_full_size_tiled_and_native(pk, kind, shape):
    """configs[4]: M = 512 on all four Llama-3-70B linears -- the default pick, EVERY tiled / wide32 kernel with K split
    1 / 2 / 4 and, for MXFP4, every native-FP4 kernel (both activation formats, K split 1 / 2) at its own tolerance plus
    the class defaults (solution_id -2 / -3).  gate_up (128x128 wide32, native 128x256 two-workgroup kernel) and down
    (K = 28672: the longest K walk, the only split-K default) are what bench.py times at M = 512."""
    n, k = LLAMA70B[shape]
    m = 512
    P = FullSizeProblem(pk, kind, n, k, 512 + n)
    a = P.activations(m, True, 300)
    P.check_sampled(P.run(a, True), a, True, "auto")
    pk.ops.enable_native_fp4(True)
    try:
        sols = pk.ops.get_fp4_solutions(P.hints(True), m, n, k)
        tiled = [sid for sid in sols if (sid >> 48) & 0xF in (8, 12)]       # 16x16x32 tiled and 32x32x16 wide kernels
        native = [sid for sid in sols if (sid >> 48) & 0xF in (9, 13)]
        assert any((sid >> 48) & 0xF == 12 for sid in tiled) and any((sid >> 48) & 0xF == 8 for sid in tiled)
        for sid in tiled:
            for splitk in (1, 2, 4):
                sk = (sid & ~(0xF << 60)) | (splitk << 60)
                P.check_sampled(P.run(a, True, sk), a, True, f"tiled split-K {sk:#x}")
        if kind == "mx":
            assert {(sid >> 32) & 7 for sid in native} == {2, 4, 6}
            for sid in native:
                for splitk in (1, 2):
                    sk = (sid & ~(0xF << 60)) | (splitk << 60)
                    check_native_sampled(P, P.run(a, True, sk), a, (sid >> 32) & 7, f"native {sk:#x}")
            for auto_sid, code in ((pk.SOLUTION_AUTO_NATIVE_MXFP8, 2), (pk.SOLUTION_AUTO_NATIVE_MXFP6, 4), (pk.SOLUTION_AUTO_NATIVE_MXFP4, 6)):
                picked = pk.ops.resolve_solution(P.hints(True), m, n, k, auto_sid)
                assert picked and (picked >> 48) & 0xF in (9, 13) and (picked >> 32) & 7 == code, hex(picked)
                check_native_sampled(P, P.run(a, True, auto_sid), a, code, f"native default {auto_sid} -> {picked:#x}")
        else:
            # NVFP4 weights (round 6): the same kernels on the MFMA-native image of the weights -- refused while no image is attached, then every
            # enumerated kernel (K split 1 / 2) and the three sentinels through the reference's own entry point
            assert {(sid >> 32) & 7 for sid in native} == {2, 4, 6} and all((sid >> 48) & 0xF == 13 and (sid >> 28) & 0xF == 1 for sid in native)
            assert P._image is None
            with pytest.raises(RuntimeError):
                pk.mul_nvfp4_a16(from_bits(a, torch.bfloat16).to(DEV), P.b, P.sp, P.gsd, m, n, k, native[0])
            assert torch.equal(pk.mul_nvfp4_a16(from_bits(a, torch.bfloat16).to(DEV), P.b, P.sp, P.gsd, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP8),
                               P.run(a, True))         # (no image attached: -2 reads as the library default, as in the reference)
            for sid in native:
                for splitk in (1, 2):
                    sk = (sid & ~(0xF << 60)) | (splitk << 60)
                    check_native_sampled(P, P.run(a, True, sk), a, (sid >> 32) & 7, f"nv native {sk:#x}")
            for auto_sid, code in ((pk.SOLUTION_AUTO_NATIVE_MXFP8, 2), (pk.SOLUTION_AUTO_NATIVE_MXFP6, 4), (pk.SOLUTION_AUTO_NATIVE_MXFP4, 6)):
                picked = pk.ops.resolve_solution(P.hints(True), m, n, k, auto_sid)
                assert picked and (picked >> 48) & 0xF == 13 and (picked >> 32) & 7 == code and (picked >> 28) & 0xF == 1, hex(picked)
                check_native_sampled(P, P.run(a, True, auto_sid), a, code, f"nv native default {auto_sid} -> {picked:#x}")
    finally:
        pk.ops.enable_native_fp4(False)


def test_native_class_table_rows_sampled(pk):
    """csrc/tuned_native_gfx950.inc beyond the four Llama-3-70B shapes (rows from the in-library tuner over seven model families): a seeded
    sample of rows per activation format, each run through the class sentinel at the row's shape and M and checked like every native kernel --
    exact semantics on the CPU-quantised activations, the class tolerance against the unquantised oracle -- and the resolved id IS the row's."""
    import re
    rows = re.findall(r"\{(\d+), (\d+), (\d+)u, (\d+)u, (\d+)u, (\d+)u, 0x([0-9a-f]+)ull\}", (ROOT / "petit-kernel_amd/csrc/tuned_native_gfx950.inc").read_text())
    rows = [(int(at), int(n), int(k), int(lo), int(hi), int(sol, 16), int(bt)) for at, bt, n, k, lo, hi, sol in rows]
    assert len(rows) > 2000
    rng = np.random.default_rng(404)
    sentinels = {2: pk.SOLUTION_AUTO_NATIVE_MXFP8, 4: pk.SOLUTION_AUTO_NATIVE_MXFP6, 6: pk.SOLUTION_AUTO_NATIVE_MXFP4}
    ran = 0
    for code, sentinel in sentinels.items():
        pool = [r for r in rows if (r[5] >> 32) & 7 == code and r[0] == 5 and r[1] * r[2] <= 160e6 and (r[1], r[2]) not in LLAMA70B.values()]
        # three rows of the MXFP4 family and (round 6) one of the NVFP4 family -- the kernels that run on the weights' MFMA-native image
        picks = [pool[i] for i in rng.choice(len(pool), len(pool), replace=False)]
        # (NVFP4 rows: every bucket has its own measured row -- taken at the M it was measured at, the upper end of a bucket up to 1024)
        # (a row is taken at the M it was measured at: the upper end of its bucket, up to 1024 -- at another M of a prefill bucket the K-split guard may differ)
        picks = [r for r in picks if r[6] == 7 and r[4] <= 1024][:3] + [r for r in picks if r[6] == 3 and r[4] <= 1024][:1]
        assert len(picks) == 4
        for at, n, k, lo, hi, sol, bt in picks:
            m = hi
            P = FullSizeProblem(pk, "mx" if bt == 7 else "nv", n, k, 7000 + n + k)
            picked = pk.ops.resolve_solution(P.hints(True), m, n, k, sentinel)
            assert picked == sol, (n, k, m, hex(picked), hex(sol))
            a = P.activations(m, True, 7100 + m)
            check_native_sampled(P, P.run(a, True, sentinel), a, code, f"native table row {n}x{k} M={m} -> {sol:#x}")
            ran += 1
            del P
            torch.cuda.empty_cache()
    assert ran == 12


def sampled_rows(m: int):
    """None (check every row) up to M = 1024; above: ~200 rows -- the first and last 32, the rows either side of every 256-row tile boundary near
    the middle and the end (the tallest workgroup tile is 256 rows), and seeded others."""
    if m <= 1024:
        return None
    edges = [r for b in (256, m // 2 // 256 * 256, (m - 1) // 256 * 256) for r in (b - 1, b, b + 1, b + 127, b + 128)]
    rows = np.concatenate([np.arange(32), np.arange(m - 32, m), np.array(edges), np.random.default_rng(m).integers(0, m, 120)])
    return np.unique(rows[(rows >= 0) & (rows < m)])


def test_bench_cells_parity(pk):
    """Every cell bench.py times (tools/benchlib.py bench_cell_plan(): the SAME list) is run here through the same call --
    solution_id -1, or -2 / -3 for the native class -- at full size and checked: zero in -> zero out, one-hot rows read back
    exact weight columns, 64 sampled output columns (first and last n-tile included) against the oracle."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import benchlib as BL
    full_plan = BL.bench_cell_plan()
    assert [c["mode"] for c in full_plan if c["shape"] == "mlp"] == ["mlp_" + m_ for m_ in BL.MlpBlock.MODES]   # -> test_bench_mlp_block_cells
    assert {c["mode"] for c in full_plan if c["shape"] == "tp8_qkv_3x1280"} == {"separate", "grouped"}         # -> test_grouped_launch
    assert [(c["M"], c["mode"]) for c in full_plan if c["shape"] == "tp8_layer"] == [(1, "layer"), (16, "layer")]                                # -> test_bench_tp8_layer_cells
    every = [c for c in full_plan if not c["mode"].startswith("hipblaslt") and c["shape"] in BL.ALL_SHAPES]
    # TP = 8 (round 6): the shard shapes of the reference's own list (tools/benchmarks/matmul.py:18-33) at decode and small-batch M, exact class
    assert {(c["shape"], c["M"]) for c in every if c["shape"] in BL.TP8} == {(s_, m_) for s_ in BL.TP8_ORDER for m_ in (1, 16, 64, 512)}
    assert all((c["a"], c["w"], c["mode"]) == ("bf16", "nv", "auto") for c in every if c["shape"] in BL.TP8)
    plan = [c for c in every if c["shape"] in BL.LLAMA70B]
    assert {(c["a"], c["w"]) for c in plan} == {("bf16", "nv"), ("fp16", "nv"), ("fp16", "mx"), ("bf16", "mx")}
    mid, pre = set(BL.MID_MS), set(BL.PREFILL_MS)
    assert mid == {32, 44, 64, 128} and pre == {1024, 2084, 4314, 16375}   # the reference's representative M list, tools/benchmarks/matmul.py:8-90
    assert {c["M"] for c in plan if (c["a"], c["w"], c["mode"]) == ("bf16", "mx", "auto")} == {1, 16, 512} | mid | pre   # the reference's only MX activation type
    assert {c["M"] for c in plan if (c["a"], c["w"], c["mode"]) == ("bf16", "nv", "auto")} == {1, 4, 8, 16, 512} | mid | pre   # configs[1..2] + M = 512 + mid M + prefill
    assert {(c["w"], c["mode"]) for c in plan if c["mode"].startswith("native")} == {(w_, "native_" + f_) for w_ in ("nv", "mx") for f_ in ("mxfp8", "mxfp6", "mxfp4")}
    assert {c["M"] for c in plan if c["mode"].startswith("native")} == {512} | pre
    # the largest cell stays inside what one 32-bit buffer descriptor / grid can address (csrc/api.hip gemm_impl refuses beyond: test_layout_and_abi)
    assert max(pre) * max(nk[0] for nk in BL.LLAMA70B.values()) * 2 < 1 << 32 and max(pre) * max(nk[1] for nk in BL.LLAMA70B.values()) < 1 << 32
    ran = 0
    plan = every
    acts = {}   # activations are a function of (M, K, dtype) only: drawn once per K (half of this test's time was CPU random numbers for 16375 x K matrices)
    for shape in BL.SHAPE_ORDER + BL.TP8_ORDER:
        n, k = BL.ALL_SHAPES[shape]
        if any(key[1] != k for key in acts):
            acts.clear()
        for w in ("nv", "mx"):
            cells = [c for c in plan if c["shape"] == shape and c["w"] == w]
            if not cells:
                continue
            P = FullSizeProblem(pk, w, n, k, 7 * n + k + len(w))
            for c in cells:
                m, is_bf16, mode = c["M"], c["a"] == "bf16", c["mode"]
                if (m, k, is_bf16) not in acts:
                    acts[(m, k, is_bf16)] = P.activations(m, is_bf16, 900 + m)
                a = acts[(m, k, is_bf16)]
                # prefill cells: the GEMM runs at its full M; the oracle checks a sample of its rows (first / last m-tiles of every tile height the
                # kernels use, the ragged tail, seeded others) x the sampled columns -- the CPU side of a 16375-row check would take minutes per cell
                rows = sampled_rows(m)
                sel = (lambda t: t) if rows is None else (lambda t: t[torch.from_numpy(rows).to(t.device)] if isinstance(t, torch.Tensor) else t[rows])
                tag = f"{shape} M={m} {c['a']}x{c['w']} {mode}"
                if mode == "auto":
                    picked = pk.ops.resolve_solution(P.hints(is_bf16), m, n, k, -1)
                    assert picked and (picked >> 48) & 0xF not in (9, 13), tag
                    if m > 512:   # the arch table's open-ended bucket must not hand a prefill chunk a K split whose slabs outgrow the operands
                        assert pk.ops.workspace_bytes(P.hints(is_bf16), m, n, k, -1) <= BL.alg_bytes(m, n, k, 16 if w == "nv" else 32), tag
                    P.check_properties(min(m, 1024), is_bf16)
                    P.check_sampled(sel(P.run(a, is_bf16)), sel(a), is_bf16, f"{tag} -> {picked:#x}")
                else:
                    sid, code = {"native_mxfp8": (pk.SOLUTION_AUTO_NATIVE_MXFP8, 2), "native_mxfp6": (pk.SOLUTION_AUTO_NATIVE_MXFP6, 4),
                                 "native_mxfp4": (pk.SOLUTION_AUTO_NATIVE_MXFP4, 6)}[mode]
                    picked = pk.ops.resolve_solution(P.hints(is_bf16), m, n, k, sid)
                    assert picked and (picked >> 32) & 7 == code and (picked >> 28) & 0xF == (1 if w == "nv" else 2), tag
                    assert torch.count_nonzero(P.run(np.zeros_like(a), is_bf16, sid)) == 0, tag
                    # a ragged prefill M may run as bulk (in the class) + a short tail through the EXACT default pick (petit_gemm_row_split): the tail rows are
                    # held to the exact class's bound, the bulk rows to the native class's
                    m1 = pk.ops.auto_row_split(P.hints(is_bf16), m, n, k, solution_id=sid)
                    assert m1 == 0 or (m - 128 <= m1 < m and m1 % 128 == 0), (tag, m1)
                    cfull = P.run(a, is_bf16, sid)
                    if m1 == 0:
                        check_native_sampled(P, sel(cfull), sel(a), code, f"{tag} -> {picked:#x}")
                    else:
                        rr = np.arange(m) if rows is None else rows
                        bulk, tail = rr[rr < m1], rr[rr >= m1]
                        pick = lambda t, idx: t[torch.from_numpy(idx).to(t.device)] if isinstance(t, torch.Tensor) else t[idx]
                        check_native_sampled(P, pick(cfull, bulk), pick(a, bulk), code, f"{tag} -> {picked:#x} (bulk rows < {m1})")
                        P.check_sampled(pick(cfull, tail), pick(a, tail), is_bf16, f"{tag}: tail rows >= {m1} through the exact default")
                ran += 1
                del a
            del P
            torch.cuda.empty_cache()
    assert ran == len(plan)


def test_prefill_default_picks_run_at_compute_speed(pk):
    """A perf regression guard, not a benchmark: round 5 found 33 prefill rows of the fp16 x MXFP4 family naming the streaming reference kernel (10 ms where the
    tiled kernels take 1.0: the tuner's output check had rejected everything else), in a family x regime no bench cell and no test timed.  Every family's default
    pick at M = 4096 on a long-K and a wide shape must reach 500 TFLOP/s (they measure 900-1400; the bug read ~100)."""
    m = 4096
    for kind in ("nv", "mx"):
        for n, k in ((8192, 28672), (10240, 8192)):
            P = FullSizeProblem(pk, kind, n, k, 5 * n + k)
            for is_bf16 in (True, False):
                dtype = torch.bfloat16 if is_bf16 else torch.float16
                x = (torch.randn((m, k), device=DEV) * 0.05).to(dtype)
                for _ in range(2):
                    P.mul(x, P.b, P.sp, P.gsd, m, n, k, -1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    P.mul(x, P.b, P.sp, P.gsd, m, n, k, -1)
                e1.record()
                torch.cuda.synchronize()
                tflops = 3 * 2.0 * m * n * k / (e0.elapsed_time(e1) * 1e-3) / 1e12
                picked = pk.ops.resolve_solution(P.hints(is_bf16), m, n, k, -1)
                assert tflops >= 500.0, f"{'bf16' if is_bf16 else 'fp16'} x {kind} {n}x{k} M={m}: {tflops:.0f} TFLOP/s with {picked:#x}"
            del P
            torch.cuda.empty_cache()


def test_raster_band_changes_the_order_not_the_result(pk):
    """csrc/device_common.hpp tile_of_block: the large-M kernels map blockIdx to C tiles XCD by XCD in bands of `ph` m-tiles ($PETIT_AMD_RASTER_BAND
    overrides the per-kernel choice; read once per process, hence child processes).  Any band -- whole columns (0), one that does not divide the
    m-tile count (3 of 9), one taller than the grid (64) -- and the default must give bit-identical outputs for the same kernel: every tile is
    computed exactly once by exactly the same code; and the default's output matches the oracle in the parent process's tests (bench cells at
    M = 2084 / 4314 / 16375: ragged last bands)."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, hashlib
sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s')
import torch
import petit_kernel as pk
m, n, k = 1100, 3584, 2048          # 9 m-tiles of 128 rows (a ragged last tile), 14 n-tiles of 256 columns
g = torch.Generator().manual_seed(11)
a = torch.randn((m, k), generator=g).bfloat16().cuda()
q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8).cuda()
gs = torch.tensor([0.5], device='cuda')
out = []
for kind in ('nv', 'mx'):
    if kind == 'nv':
        s = (torch.rand((n, k // 16), generator=g) * 3.5 + 0.25).to(torch.float8_e4m3fn).cuda()
        b, sp, mul = pk.repack_nvfp4(q.view(torch.int32), n, k), pk.process_nvfp4_scales(s, n, k), pk.mul_nvfp4_a16
        fmt = pk.DataType.float4_e2m1
    else:
        s = torch.randint(119, 136, (n, k // 32), generator=g, dtype=torch.uint8).cuda()
        b, sp, mul = pk.repack_mxfp4(q.view(torch.int32), n, k), pk.process_mxfp4_scales(s, n, k), pk.mul_mxfp4_a16
        fmt = pk.DataType.mxfloat4_e2m1
    h = pk.PetitSolutionHints(); h.a_type = h.c_type = torch.bfloat16; h.b_type = fmt
    ids = [int(sid) for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF in (8, 12) and (sid >> 60) == 1]   # tiled / wide32 / shared-unpack, unsplit
    assert len(ids) >= 10
    for sid in ids:
        c = mul(a, b, sp, gs, m, n, k, sid)
        out.append('%%s %%x %%s' %% (kind, sid, hashlib.sha256(c.view(torch.int16).cpu().numpy().tobytes()).hexdigest()))
    if kind == 'mx':
        c = pk.mul_mxfp4_native(a, b, sp, gs, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP8)
        out.append('native8 %%s' %% hashlib.sha256(c.view(torch.int16).cpu().numpy().tobytes()).hexdigest())
print('\n'.join(out))
""" % (ROOT / "petit-kernel_amd", ROOT)
    results = {}
    for band in ("default", "0", "3", "64"):
        env = {k_: v for k_, v in os.environ.items() if k_ != "PETIT_AMD_RASTER_BAND"}
        if band != "default":
            env["PETIT_AMD_RASTER_BAND"] = band
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        results[band] = [ln for ln in out.stdout.strip().splitlines() if ln.startswith(("nv ", "mx ", "native8 "))]
        assert len(results[band]) >= 21
    assert results["0"] == results["default"] and results["3"] == results["default"] and results["64"] == results["default"]


def test_auto_row_split_matches_oracle(pk):
    """A default-pick call at a ragged prefill M runs as bulk + tail (csrc/api.hip plan_row_split, petit_gemm_auto_row_split): both launches write their
    row ranges of C, the scratch the library asks for covers both, and every row -- the boundary rows of the split, the tail, sampled bulk rows -- matches
    the oracle; with bias and with the SiLU-mul epilogue (C has n / 2 columns: the tail's row offset follows).  An explicit id never splits."""
    cases = [("nv", 8192, 8192, 1100, True), ("nv", 8192, 8192, 2084, True), ("mx", 8192, 28672, 2084, True), ("nv", 8192, 8192, 600, False),
             ("nv", 8192, 28672, 2200, True)]
    ran = 0
    for kind, n, k, m, is_bf16 in cases:
        P = FullSizeProblem(pk, kind, n, k, 31 * n + k + m)
        h = P.hints(is_bf16)
        m1 = pk.ops.auto_row_split(h, m, n, k)
        if not m1:
            continue   # (the arch table changed under this case: the others still cover the path)
        assert 0 < m1 < m and pk.ops.auto_row_split(h, m1, n, k) == 0, (kind, n, k, m, m1)
        need = pk.ops.workspace_bytes(h, m, n, k, -1)
        assert need >= max(pk.ops.workspace_bytes(h, m1, n, k, -1), 0) and need <= 4 * m * n * 4
        a = P.activations(m, is_bf16, 77 + m)
        rows = np.unique(np.concatenate([np.arange(m1 - 40, min(m, m1 + 140)), np.arange(m - 32, m), np.arange(32), np.random.default_rng(m).integers(0, m, 64)]))
        sel = torch.from_numpy(rows).to(DEV)
        c = P.run(a, is_bf16)
        P.check_sampled(c[sel], a[rows], is_bf16, f"row split {kind} {n}x{k} M={m} -> {m1} + {m - m1}")
        # the same through the explicit id of the whole problem's pick (one launch): same numbers up to the kernels' summation order
        sid = pk.ops.resolve_solution(h, m, n, k, -1)
        c1 = P.run(a, is_bf16, sid)
        assert torch.allclose(c[sel].float(), c1[sel].float(), rtol=2e-2, atol=2e-2 * float(c1.float().abs().mean()))
        del c1
        # bias + SiLU-mul
        dtype = torch.bfloat16 if is_bf16 else torch.float16
        x = from_bits(a, dtype).to(DEV)
        bias = torch.randn(n, dtype=dtype, device=DEV)
        cb = P.mul(x, P.b, P.sp, P.gsd, m, n, k, -1, bias=bias)
        assert torch.allclose(cb[sel].float(), (c[sel].float() + bias.float()), rtol=2e-2, atol=2e-2 * float(c.float().abs().mean()) + 0.05)
        if pk.ops.auto_row_split(h, m, n, k, activation="silu_mul"):
            hs = P.mul(x, P.b, P.sp, P.gsd, m, n, k, -1, activation="silu_mul")
            assert hs.shape == (m, n // 2)
            g, u = c[sel, : n // 2].float(), c[sel, n // 2:].float()
            want = g * torch.sigmoid(g) * u
            assert torch.allclose(hs[sel].float(), want, rtol=3e-2, atol=3e-2 * float(want.abs().mean()) + 1e-3), f"silu_mul {kind} {n}x{k} M={m}"
        ran += 1
        del P, c, cb, x
        torch.cuda.empty_cache()
    assert ran >= 2


def test_native_row_split_is_its_two_parts_and_is_capturable(pk):
    """The native class at a ragged prefill M (csrc/pick.hip plan_row_split_native): the call's bulk rows are bit for bit what the class computes on a problem of
    those rows alone, its tail rows bit for bit what the EXACT default pick computes on the tail alone (never another accuracy class, never a different kernel than the
    queries name), and the whole call -- quantiser + class kernel + exact kernel -- replays from a HIP graph to the same bits."""
    ran = 0
    for kind in ("nv", "mx"):
        n, k, m = 8192, 8192, 2084
        P = FullSizeProblem(pk, kind, n, k, 9100 + len(kind))
        h = P.hints(True)
        for sid in (pk.SOLUTION_AUTO_NATIVE_MXFP8, pk.SOLUTION_AUTO_NATIVE_MXFP4):
            if kind == "nv":
                _ = P.image
            m1 = pk.ops.auto_row_split(h, m, n, k, solution_id=sid)
            if not m1:
                continue   # (the class table changed under this case)
            assert 0 < m - m1 <= 128 and pk.ops.auto_row_split(h, m1, n, k, solution_id=sid) == 0
            a = P.activations(m, True, 9200)
            c = P.run(a, True, sid)
            bulk = P.run(a[:m1], True, sid)
            tail = P.run(a[m1:], True, -1)
            assert torch.equal(c[:m1].view(torch.int16), bulk.view(torch.int16)), (kind, sid)
            assert torch.equal(c[m1:].view(torch.int16), tail.view(torch.int16)), (kind, sid)
            P.check_sampled(c[m1:], a[m1:], True, f"native row split, exact tail {kind}")
            x = from_bits(a, torch.bfloat16).to(DEV)
            mul = P.mul if kind == "nv" else pk.mul_mxfp4_native
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                warm = mul(x, P.b, P.sp, P.gsd, m, n, k, sid)   # (scratch grown outside the capture)
                st.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    out = mul(x, P.b, P.sp, P.gsd, m, n, k, sid)
                out.zero_()
                g.replay()
                st.synchronize()
            assert torch.equal(out.view(torch.int16), c.view(torch.int16)) and torch.equal(warm.view(torch.int16), c.view(torch.int16)), (kind, sid)
            ran += 1
            del c, bulk, tail, out, warm, g
        if kind == "mx":
            # the process-wide default class: AUTO on MXFP4 weights plans the same bulk + tail, and the queries say so
            prev = pk.ops.mxfp4_default_activations()
            pk.ops.set_mxfp4_default_activations("mxfp8")
            try:
                m1 = pk.ops.auto_row_split(h, m, n, k)
                assert m1, "default class: no row split"
                a = P.activations(m, True, 9300)
                c = P.run(a, True, -1)
                bulk = P.run(a[:m1], True, -1)
                tail = P.run(a[m1:], True, -1)
                assert torch.equal(c[:m1].view(torch.int16), bulk.view(torch.int16))
                assert torch.equal(c[m1:].view(torch.int16), tail.view(torch.int16))
                del c, bulk, tail
            finally:
                pk.ops.set_mxfp4_default_activations(prev)
        del P
        torch.cuda.empty_cache()
    assert ran >= 2


def test_bench_mlp_block_cells(pk):
    """The gated-MLP cells of bench.py (tools/benchlib.py MlpBlock: Llama-3-70B gate_up -> SiLU-mul -> down at M = 512, MXFP4
    weights) at full size, through the same calls: the exact path against the oracle (sampled columns of h, then `down` on the
    GPU's own h), the native pipelines against the exact result at the class tolerance and against each other."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import benchlib as BL
    m, hid, inter = 512, 8192, 28672
    P1 = FullSizeProblem(pk, "mx", 2 * inter, hid, 4001)
    P2 = FullSizeProblem(pk, "mx", hid, inter, 4002)
    x_bits = P1.activations(m, True, 4003)
    x = from_bits(x_bits, torch.bfloat16).to(DEV)
    gs = P1.gsd
    h = pk.mul_mxfp4_a16(x, P1.b, P1.sp, gs, m, 2 * inter, hid, -1, activation="silu_mul")
    cols = np.unique(np.random.default_rng(5).integers(0, inter, 48))
    dq = O.dequant_mxfp4(np.concatenate([P1.q[cols], P1.q[cols + inter]]), np.concatenate([P1.s[cols], P1.s[cols + inter]])).astype(np.float64)
    y1 = to_f32(x_bits, True).astype(np.float64) @ dq.T * P1.gs
    g, u = y1[:, : len(cols)], y1[:, len(cols):]
    want = g / (1.0 + np.exp(-g)) * u
    got = h[:, torch.from_numpy(cols).to(DEV)].float().cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 2e-2 * np.abs(want) + 2e-2 * np.sqrt(np.mean(want ** 2))).all()
    y_exact = pk.mul_mxfp4_a16(h, P2.b, P2.sp, P2.gsd, m, hid, inter, -1)
    P2.check_sampled(y_exact, bits(h), True, "down on the GPU's h")
    ye = y_exact.float()
    rms = ye.pow(2).mean().sqrt().item()
    outs = {}
    for fmt, sid in (("mxfp4", pk.SOLUTION_AUTO_NATIVE_MXFP4), ("mxfp8", pk.SOLUTION_AUTO_NATIVE_MXFP8), ("mxfp6", pk.SOLUTION_AUTO_NATIVE_MXFP6)):
        h4 = pk.mul_mxfp4_native(x, P1.b, P1.sp, gs, m, 2 * inter, hid, sid, activation="silu_mul")
        outs[fmt + "_4launch"] = pk.mul_mxfp4_native(h4, P2.b, P2.sp, P2.gsd, m, hid, inter, sid).float()
        hq = pk.mul_mxfp4_native(pk.quantize_activations(x, fmt), P1.b, P1.sp, gs, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=fmt)
        outs[fmt + "_pipeline"] = pk.mul_mxfp4_native(hq, P2.b, P2.sp, P2.gsd, m, hid, inter, sid).float()
    for name, y in outs.items():
        rel = (y - ye).pow(2).mean().sqrt().item() / rms
        assert rel <= (0.45 if "mxfp4" in name else 0.08), (name, rel)
    for fmt, tol in (("mxfp4", 0.12), ("mxfp8", 0.03), ("mxfp6", 0.03)):
        rel = (outs[fmt + "_pipeline"] - outs[fmt + "_4launch"]).pow(2).mean().sqrt().item() / rms
        assert rel <= tol, (fmt, rel)


@pytest.mark.parametrize("m", [1, 16])
def test_bench_tp8_layer_cells(pk, m):
    """bench.py's `tp8_layer` cells (tools/benchlib.py DecodeLayerTP8: the four GEMM launches of one Llama-3-70B layer on one GPU of a TP = 8 deployment, chained)
    through the same calls: every stage against the oracle on the GPU's own input of that stage (sampled output columns; the grouped q / k / v launch is
    compared bit for bit with separate calls in test_grouped_launch)."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import benchlib as BL
    L = BL.DecodeLayerTP8(m, DEV, rotate_mb=64)
    q, k_, v, o, h, y = L.run(1)
    torch.cuda.synchronize()
    gs = float(L.gs.item())
    rng = np.random.default_rng(17 + m)

    def unpacked(wts, i, n, kk):
        # (the bench draws PACKED bytes: any bytes are a valid weight matrix -- read them back through the layout model)
        from oracle import cdna4_layout as LY
        b, sp = wts[i]
        qw = LY.unpack_weights(b.cpu().numpy().view(np.uint32).ravel(), n, kk)
        sc = LY.unpack_nvscales(sp.view(torch.uint8).cpu().numpy().ravel(), n, kk)
        return qw.view(np.uint8).reshape(n, kk // 2), sc

    def check(out, x, wts, n, kk, act=False, tag=""):
        qb, sb = unpacked(wts, 1, n, kk)
        n_out = n // 2 if act else n
        cols = np.unique(np.concatenate([rng.integers(0, n_out, 40), [0, n_out - 1]]))
        xb = bits(x)
        if act:
            dq = O.dequant_nvfp4(np.concatenate([qb[cols], qb[cols + n_out]]), np.concatenate([sb[cols], sb[cols + n_out]])).astype(np.float64)
            y1 = to_f32(xb, True).astype(np.float64) @ dq.T * gs
            g, u = y1[:, : len(cols)], y1[:, len(cols):]
            want = g / (1.0 + np.exp(-g)) * u
            got = out[:, torch.from_numpy(cols).to(DEV)].float().cpu().numpy().astype(np.float64)
            assert (np.abs(got - want) <= 2e-2 * np.abs(want) + 2e-2 * np.sqrt(np.mean(want ** 2)) + 1e-6).all(), tag
        else:
            _, want = O.gemm_ref(xb, True, O.dequant_nvfp4(qb[cols], sb[cols]), gs)
            check_gemm(bits(out[:, torch.from_numpy(cols).to(DEV)]), want, True)

    check(q, L.x, L.wq, 1024, 8192, tag="q")
    check(k_, L.x, L.wk, 128, 8192, tag="k")
    check(v, L.x, L.wv, 128, 8192, tag="v")
    check(o, q, L.wo, 8192, 1024, tag="o")
    check(h, o, L.wgu, 7168, 8192, act=True, tag="gate_up + SiLU-mul")
    check(y, h, L.wd, 8192, 3584, tag="down")


# the kernels whose step-ending wait is a counted `s_waitcnt vmcnt(N)` + raw `s_barrier` (a wrong count is a timing-dependent
# race that one parity pass can miss) and every cross-workgroup K split (slabs + fixed-order reduce): all deterministic by
# design, so ANY bit difference between two launches of the same kernel on the same inputs is a bug.
REPEAT_PROBLEMS_SMALL_M = [(16, 512, 8192), (11, 272, 4096), (5, 96, 3072), (16, 128, 1536), (9, 64, 768)]
REPEAT_PROBLEMS_LARGE_M = [(512, 1024, 4096), (130, 416, 2048), (33, 96, 1024), (70, 128, 1536)]


@pytest.mark.parametrize("kind", ["nv", "mx"])
def test_repeat_launch_bit_identical(pk, kind):
    """tools/probes/mid_race.py + native_race.py as a test: the shared-activation-tile kernels (gemm_mid.hpp), the wide32
    kernels (PF = 2: loads in flight across the barrier), both native kernels, and every K split (stream, tiled, wide32,
    native: split 2 and 4), 30 launches each on several problems incl. ragged M / N, other traffic in between so that timing
    varies: every launch bit-identical to the first, and the first within the parity bound of the oracle."""
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
    junk = torch.empty(48 << 20, dtype=torch.uint8, device=DEV)
    pk.ops.enable_native_fp4(True)
    launches = 0
    try:
        for (m, n, k) in REPEAT_PROBLEMS_SMALL_M + REPEAT_PROBLEMS_LARGE_M:
            if kind == "mx" and n % 32:
                continue
            a_bits, q, s, gs = random_problem(kind, m, n, k, 31337 + m + n + k, True)
            a = from_bits(a_bits, torch.bfloat16).to(DEV)
            qd = torch.from_numpy(q).to(DEV)
            gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
            b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
            if kind == "nv":
                sp, mul = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k), pk.mul_nvfp4_a16
            else:
                sp, mul = pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k), pk.mul_mxfp4_a16
            ref = oracle_ref(kind, a_bits, True, q, s, gs)
            sum_abs = oracle_sum_abs(kind, a_bits, True, q, s, gs)
            if kind == "nv":    # the native kernels of the NVFP4 family run on the weights' MFMA-native image (explicit ids find it attached to b)
                pk.attach_nvfp4_native(b, pk.nvfp4_native_image(b, sp, n, k))
            cands = []
            for sid in pk.ops.get_fp4_solutions(h, m, n, k):
                code, wm = (sid >> 48) & 0xF, (sid >> 36) & 0xF
                counted = wm == 2 or code in (9, 12, 13)
                if counted:
                    cands.append(sid)
                if code in (0, 8, 9, 12, 13) and m > 16 or (code == 0 and wm == 1):
                    cands += [(sid & ~(0xF << 60)) | (sk << 60) for sk in (2, 4)]
            assert cands
            for sid in cands:
                first = mul(a, b, sp, gsd, m, n, k, sid).clone()
                if (sid >> 48) & 0xF not in (9, 13):        # (the native class has its own tolerance: tested elsewhere)
                    check_gemm(bits(first), ref, True, sum_abs)
                for it in range(30):
                    if it % 3 == 0:
                        junk.add_(1)
                    c = mul(a, b, sp, gsd, m, n, k, sid)
                    assert torch.equal(c.view(torch.int16), first.view(torch.int16)), f"{sid:#x} m={m} n={n} k={k}: launch {it} differs"
                    launches += 1
            if kind == "nv":
                pk.attach_nvfp4_native(b, None)
    finally:
        pk.ops.enable_native_fp4(False)
    assert launches >= 3000


def test_split_k8_ids_through_both_bindings(pk):
    """A K split of 8..15 sets bit 63 of the id (round-2 ADVICE: the compiled op's `int solution_id` is a signed int64 and
    refused such ids; 23 arch-table rows carry split 8): the same id through the compiled op and the ctypes layer, bit-identical
    results, within the oracle bound."""
    from petit_kernel import compiled, ops
    m, n, k = 130, 256, 16384
    a_bits, q, s, gs = random_problem("nv", m, n, k, 880, True)
    ref = oracle_ref("nv", a_bits, True, q, s, gs)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1
    tiled = next(x for x in pk.ops.get_fp4_solutions(h, m, n, k) if (x >> 48) & 0xF == 8)
    sid = (tiled & ~(0xF << 60)) | (8 << 60)
    assert sid >= 1 << 63
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    b = ops.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = ops.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    c1 = ops.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid)
    check_gemm(bits(c1), ref, True)
    assert compiled.available(), compiled.why_unavailable()
    c2 = compiled.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid)
    assert torch.equal(c1.view(torch.int16), c2.view(torch.int16))
    c3 = pk.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid)            # the package front end (whichever binding it chose)
    assert torch.equal(c1.view(torch.int16), c3.view(torch.int16))
    with pytest.raises(RuntimeError, match="No kernel implementation"):
        compiled.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid ^ (0xF << 48))   # an unknown id with bit 63 set: refused, not misread as AUTO


def test_python_scratch_is_per_call_on_every_stream(pk):
    """Round-2 ADVICE: once set_workspace() had been called, the ctypes layer stopped allocating per-call scratch and the
    registered buffer, bound to the first stream, was refused on any other (BAD_ARGUMENT for an explicit K-split id, a silent
    slower kernel for AUTO) -- e.g. on the side stream torch.cuda.graph captures on.  Both Python layers now always hand
    every call its own scratch; the registered workspace serves raw C callers only."""
    from petit_kernel import compiled, ops
    m, n, k = 24, 256, 4096
    a_bits, q, s, gs = random_problem("nv", m, n, k, 8101, True)
    ref = oracle_ref("nv", a_bits, True, q, s, gs)
    a = from_bits(a_bits, torch.bfloat16).to(DEV)
    b = ops.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = ops.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.float4_e2m1
    sid = next(x for x in pk.ops.get_fp4_solutions(h, m, n, k) if (x >> 48) & 0xF == 0)
    sid = (sid & ~(0xF << 60)) | (2 << 60)
    ws = torch.empty(2 * m * n, dtype=torch.float32, device=DEV)
    ops.set_workspace(ws)
    try:
        for layer in (ops, compiled):
            outs = []
            for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
                with torch.cuda.stream(stream):
                    outs.append(layer.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid))
                stream.synchronize()
            check_gemm(bits(outs[0]), ref, True)
            assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        # and under capture on torch's side stream after an eager warm-up on the current one
        ops.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.mul_nvfp4_a16(a, b, sp, gsd, m, n, k, sid)
        g.replay()
        torch.cuda.synchronize()
        check_gemm(bits(out), ref, True)
    finally:
        ops.set_workspace(None)


def test_workspace_alignment_is_enforced(pk):
    """include/petit_amd.h "Scratch memory": a workspace pointer must be 256-byte aligned (f32x4 slabs, 16-byte activation
    loads); a misaligned one is PETIT_ERROR_BAD_ARGUMENT on both the per-call and the registered path."""
    from petit_kernel import _lib
    import ctypes as C
    m, n, k = 24, 256, 4096
    buf = torch.zeros(max(m * k, n * k, m * n), dtype=torch.int32, device=DEV)
    hints = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    ws = torch.empty(2 * m * n * 4 + 512, dtype=torch.uint8, device=DEV)
    args = (buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), m, n, k, C.byref(hints),
            C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.lib.petit_gemm_fp4_fp16_grid_ws(*args, C.c_void_p(ws.data_ptr() + 16), C.c_uint64(2 * m * n * 4), stream) == _lib.PETIT_ERROR_BAD_ARGUMENT
    assert _lib.lib.petit_gemm_fp4_fp16_grid_ws(*args, C.c_void_p(ws.data_ptr() + 256), C.c_uint64(2 * m * n * 4), stream) == 0
    assert _lib.lib.petit_set_workspace(C.c_void_p(ws.data_ptr() + 8), C.c_uint64(1024)) == _lib.PETIT_ERROR_BAD_ARGUMENT
    assert _lib.lib.petit_set_workspace(None, 0) == 0
    torch.cuda.synchronize()


def test_e8m0_zero_scale_divergence_is_pinned(pk):
    """Documented semantic difference: an e8m0 scale byte of 0 dequantises to 0.0 in the reference's GPU
    kernel (dequant.cuh:198-203 builds the bf16 bit pattern `e << 7`: exponent field 0 with a zero mantissa IS 0.0) -- which
    is what the oracle restates -- and to 2^-127 in the OCP definition that gfx950's hardware convert follows (it reads only
    the exponent field of its scale operand).  Weights of magnitude 6 under an all-zero scale tensor and activations of
    2^120 make the two readings differ visibly: every exact kernel of this build returns a * 6 * 2^-127 (bit exact), the
    oracle returns 0.  The reference's own tests only draw scale bytes 1..237, so no fixture is affected."""
    m, n, k = 2, 64, 1024
    q = np.full((n, k // 2), 0x77, dtype=np.uint8)             # every weight = +6.0
    s = np.zeros((n, k // 32), dtype=np.uint8)                 # every block scale byte = 0
    a = np.zeros((m, k), dtype=np.float32)
    a[0, 5] = 2.0 ** 120
    a[1, 77] = -(2.0 ** 118)
    a_bits = O.f32_to_bf16_bits(a)
    assert O.e8m0_to_f32(np.zeros(1, dtype=np.uint8))[0] == 0.0                       # the reference's reading
    assert not oracle_ref("mx", a_bits, True, q, s, 1.0).any()
    want = np.zeros((m, n), dtype=np.float32)                                         # the OCP / hardware reading
    want[0, :] = 6.0 * 2.0 ** (120 - 127)
    want[1, :] = -6.0 * 2.0 ** (118 - 127)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.mxfloat4_e2m1
    for sid in [-1] + list(pk.ops.get_fp4_solutions(h, m, n, k)):
        got = to_f32(run_case(pk, "mx", a_bits, True, q, s, 1.0, m, n, k, sid), True)
        assert np.array_equal(got, want), (hex(sid & (2 ** 64 - 1)), got[:, :2], want[:, :2])


# --- the native-FP4 path (opt-in): exact semantics + its own stated tolerance ---------------------

def quantize_act_mxfp8(a_f32: np.ndarray) -> np.ndarray:
    """CPU statement of quantize_act_kernel (csrc/gemm_native.hpp): per 32-k block, E8M0 scale
    2^(E-7) with E the exponent of the block maximum, elements rounded to e4m3 (RNE).  Returns the
    DEQUANTISED activations (exactly representable in bf16: 4 significant bits x power of two)."""
    m, k = a_f32.shape
    blk = a_f32.reshape(m, k // 32, 32)
    amax = np.abs(blk).max(axis=2)
    ebits = (amax.astype(np.float32).view(np.uint32) >> 23) & 0xFF
    sbyte = np.where(amax == 0, 127, np.clip(ebits.astype(np.int64) - 7, 1, 254))
    scale = np.ldexp(1.0, sbyte - 127).astype(np.float32)[:, :, None]
    q = torch.from_numpy((blk / scale).astype(np.float32)).to(torch.float8_e4m3fn).float().numpy()
    return (q * scale).reshape(m, k)


E2M1_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def quantize_act_mxfp4(a_f32: np.ndarray) -> np.ndarray:
    """CPU statement of quantize_act32_kernel<., 4> (csrc/gemm_native32.hpp): per 32-k block the OCP-MX scale
    2^(E - 2), E the exponent of the block maximum (so the maximum lands in [4, 8)), elements rounded to e2m1
    (round-to-nearest-even on the grid 0 .5 1 1.5 2 3 4 6, saturating at 6).  Returns the DEQUANTISED activations."""
    m, k = a_f32.shape
    blk = a_f32.reshape(m, k // 32, 32).astype(np.float64)
    amax = np.abs(blk).max(axis=2)
    ebits = (amax.astype(np.float32).view(np.uint32) >> 23) & 0xFF
    sbyte = np.where(amax == 0, 127, np.clip(ebits.astype(np.int64) - 2, 1, 254))
    scale = np.ldexp(1.0, sbyte - 127)[:, :, None]
    x = np.abs(blk) / scale
    # nearest grid point; ties go to the even mantissa (grid indices 0, 2, 4, 6 are the even ones)
    idx = np.searchsorted(E2M1_GRID, x, side="left").clip(1, 7)
    lo, hi = E2M1_GRID[idx - 1], E2M1_GRID[idx]
    pick_hi = (x - lo > hi - x) | ((x - lo == hi - x) & (idx % 2 == 0))
    q = np.where(x >= 6.0, 6.0, np.where(pick_hi, hi, lo))
    return (np.sign(blk) * q * scale).reshape(m, k).astype(np.float32)


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("m,n,k", [(64, 256, 1024), (130, 96, 2048), (512, 1024, 2048), (33, 64, 512), (5, 64, 1024), (1, 128, 512), (257, 160, 1280)])
def test_native_fp4_activations(pk, m, n, k, is_bf16):
    """FP4 x FP4 (MXFP4 weights raw, activations quantised on the fly to MXFP4: the 10 PFLOP/s instruction).  Opt-in,
    ids carry mfma_type 6.  (1) exact semantics: against the oracle run on the CPU-emulated MXFP4 activations the kernel
    is within the usual 1e-2 bound (only f32 summation order and the final rounding differ).  (2) stated end-to-end
    tolerance against the unquantised oracle: e2m1 carries up to 2^-2 relative error per element (plus saturation of
    block maxima in (6, 8) scale units: 25 %), so |c - ref| <= 0.12 * sum|a||w| + 1e-2 and rms error <= 25 % of the
    output rms on these random problems -- an accuracy class for experiments, never a default."""
    a_bits, q, s, gs = random_problem("mx", m, n, k, 5151 + m + n + k, is_bf16)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.mxfloat4_e2m1
    pk.ops.enable_native_fp4(True)
    try:
        fp4 = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 32) & 7 == 6]
        assert fp4 and all((sid >> 48) & 0xF == 13 for sid in fp4)
        a_f32 = to_f32(a_bits, is_bf16)
        a_q = quantize_act_mxfp4(a_f32)
        dq = O.dequant_mxfp4(q, s)
        _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq, gs)       # (4 significant bits x power of two: exact in bf16)
        _, full = O.gemm_ref(a_bits, is_bf16, dq, gs)
        sum_abs = (np.abs(a_f32) @ np.abs(dq).T) * gs
        derived = native_exact_bound(a_q, dq, gs, "mxfp4") # (the bound derived from the instruction: see native_exact_bound)
        fin = np.isfinite(full) & (np.abs(full) < (3e38 if is_bf16 else 6e4))
        for sid in fp4:
            for splitk in (1, 2):
                sk = (sid & ~(0xF << 60)) | (splitk << 60)
                c = to_f32(run_case(pk, "mx", a_bits, is_bf16, q, s, gs, m, n, k, sk), is_bf16).astype(np.float64)
                err = np.abs(c - exact)[fin]
                assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)[fin]).all(), f"{sk:#x} max {err.max()}"
                native_p99_guard(err, exact[fin], ((np.abs(a_q) @ np.abs(dq).T) * gs)[fin], f"{sk:#x}")
                assert (np.abs(c - full)[fin] <= 0.12 * sum_abs[fin] + 1e-2).all(), f"{sk:#x}"
                assert np.sqrt(np.mean((c - full)[fin] ** 2)) <= 0.25 * np.sqrt(np.mean(full[fin] ** 2)), f"{sk:#x}"
    finally:
        pk.ops.enable_native_fp4(False)


E2M3_GRID = np.array([i / 8.0 for i in range(8)] + [(1.0 + i / 8.0) * 2.0 ** e for e in range(3) for i in range(8)])


def quantize_act_mxfp6(a_f32: np.ndarray) -> np.ndarray:
    """CPU statement of quantize_act32_fp6_kernel (csrc/gemm_native32.hpp): per 32-k block the OCP-MX scale 2^(E - 2), E the exponent of the
    block maximum (so the maximum lands in [4, 8)), elements rounded to e2m3 -- round-to-nearest-even on the grid 0, 1/8 .. 7/8 (subnormals),
    1 .. 1.875, 2 .. 3.75, 4 .. 7.5, saturating at 7.5 (v_cvt_scalef32_pk32_fp6_*, tools/probes/mfma32_fp6_probe.hip).  Returns the
    DEQUANTISED activations."""
    m, k = a_f32.shape
    blk = a_f32.reshape(m, k // 32, 32).astype(np.float64)
    amax = np.abs(blk).max(axis=2)
    ebits = (amax.astype(np.float32).view(np.uint32) >> 23) & 0xFF
    sbyte = np.where(amax == 0, 127, np.clip(ebits.astype(np.int64) - 2, 1, 254))
    scale = np.ldexp(1.0, sbyte - 127)[:, :, None]
    x = np.abs(blk) / scale
    idx = np.searchsorted(E2M3_GRID, x, side="left").clip(1, 31)
    lo, hi = E2M3_GRID[idx - 1], E2M3_GRID[idx]
    pick_hi = (x - lo > hi - x) | ((x - lo == hi - x) & (idx % 2 == 0))      # ties: the even code (grid index = code)
    q = np.where(x >= 7.5, 7.5, np.where(pick_hi, hi, lo))
    return (np.sign(blk) * q * scale).reshape(m, k).astype(np.float32)


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("m,n,k", [(64, 256, 1024), (130, 96, 2048), (512, 1024, 2048), (33, 64, 512), (5, 64, 1024), (1, 128, 768), (257, 160, 1280), (200, 512, 4096)])
def test_native_mxfp6_activations(pk, m, n, k, is_bf16):
    """FP4 x FP6 (MXFP4 weights raw, activations quantised on the fly to MXFP6 e2m3: the instruction still runs at its FP4 rate, the elements carry
    e4m3's three mantissa bits).  Opt-in, ids carry mfma_type 4, sentinel -4.  (1) exact semantics: against the oracle run on the CPU-emulated
    MXFP6 activations the kernel is within the usual 1e-2 bound.  (2) stated end-to-end tolerance against the unquantised oracle: the MXFP8
    class's bounds -- e2m3 carries 2^-4 relative error per element in its three normal binades, 1/64 of the block maximum below them, and clips
    a block maximum in (7.5, 8) scale units by at most 6 %."""
    a_bits, q, s, gs = random_problem("mx", m, n, k, 6161 + m + n + k, is_bf16)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16 if is_bf16 else torch.float16
    h.b_type = pk.DataType.mxfloat4_e2m1
    pk.ops.enable_native_fp4(True)
    try:
        fp6 = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 32) & 7 == 4]
        assert fp6 and all((sid >> 48) & 0xF == 13 for sid in fp6)
        a_f32 = to_f32(a_bits, is_bf16)
        a_q = quantize_act_mxfp6(a_f32)
        dq = O.dequant_mxfp4(q, s)
        _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq, gs)       # (5 significant bits x power of two: exact in bf16)
        _, full = O.gemm_ref(a_bits, is_bf16, dq, gs)
        sum_abs = (np.abs(a_f32) @ np.abs(dq).T) * gs
        derived = native_exact_bound(a_q, dq, gs, "mxfp6") # (the bound derived from the instruction: see native_exact_bound)
        fin = np.isfinite(full) & (np.abs(full) < (3e38 if is_bf16 else 6e4))
        for sid in fp6:
            for splitk in (1, 2):
                sk = (sid & ~(0xF << 60)) | (splitk << 60)
                c = to_f32(run_case(pk, "mx", a_bits, is_bf16, q, s, gs, m, n, k, sk), is_bf16).astype(np.float64)
                err = np.abs(c - exact)[fin]
                assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)[fin]).all(), f"{sk:#x} max {err.max()}"
                native_p99_guard(err, exact[fin], ((np.abs(a_q) @ np.abs(dq).T) * gs)[fin], f"{sk:#x}")
                assert (np.abs(c - full)[fin] <= 2e-2 * sum_abs[fin] + 1e-2).all(), f"{sk:#x}"
                assert np.sqrt(np.mean((c - full)[fin] ** 2)) <= 6e-2 * np.sqrt(np.mean(full[fin] ** 2)), f"{sk:#x}"
        # the class sentinel on its own entry point: an enumerated kernel of the class, same numbers
        qd = torch.from_numpy(q).to(DEV)
        b = pk.repack_mxfp4(qd.view(torch.int32), n, k)
        sp = pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
        gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
        ad = from_bits(a_bits, h.a_type).to(DEV)
        c_auto = to_f32(bits(pk.mul_mxfp4_native(ad, b, sp, gsd, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP6)), is_bf16).astype(np.float64)
        assert (np.abs(c_auto - exact)[fin] <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)[fin]).all()
        # pre-quantised activations (one launch) are bit-identical to quantising inside the call
        qa = pk.quantize_activations(ad, "mxfp6")
        c_pre = pk.mul_mxfp4_native(qa, b, sp, gsd, m, n, k, fp6[0])
        c_fly = pk.mul_mxfp4_native(ad, b, sp, gsd, m, n, k, fp6[0])
        assert torch.equal(c_pre.view(torch.int16), c_fly.view(torch.int16))
    finally:
        pk.ops.enable_native_fp4(False)


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("m,n,k", [(64, 256, 1024), (130, 96, 2048), (512, 1024, 2048), (33, 64, 512), (5, 64, 1024), (1, 128, 512), (257, 160, 1280)])
def test_native_mxfp4(pk, m, n, k, is_bf16):
    a_bits, q, s, gs = random_problem("mx", m, n, k, 4242 + m + n + k, is_bf16)
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = dtype
    h.b_type = pk.DataType.mxfloat4_e2m1
    pk.ops.enable_native_fp4(False)
    assert all((sid >> 32) & 7 != 2 for sid in pk.ops.get_fp4_solutions(h, m, n, k))   # opt-in only
    pk.ops.enable_native_fp4(True)
    try:
        native = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 32) & 7 == 2]
        assert native
        pk.ops.set_workspace(None)
        # the C ABI without any scratch (none registered, none passed) refuses a native kernel; the Python layer hands
        # every call its own scratch, and a registered workspace (round-1 style) is honoured when there is one
        from petit_kernel import _lib
        import ctypes as C
        ch = _lib.SolutionHints(_lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_MXFP4_E2M1,
                                _lib.CXX_DTYPE_BF16 if is_bf16 else _lib.CXX_DTYPE_FP16, 0)
        dummy = torch.zeros(max(m * k, n * k, m * n), dtype=torch.int32, device=DEV)
        assert _lib.lib.petit_gemm_mxfp4_fp16_grid(dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(),
                                                   m, n, k, C.byref(ch), C.c_uint64(native[0]), None) == _lib.PETIT_ERROR_KERNEL_SHAPE
        assert pk.ops.workspace_bytes(h, m, n, k, native[0]) == pk.ops.native_workspace_bytes(m, k)
        c_percall = run_case(pk, "mx", a_bits, is_bf16, q, s, gs, m, n, k, native[0])      # per-call scratch
        ws = torch.empty(pk.ops.native_workspace_bytes(m, k), dtype=torch.uint8, device=DEV)
        pk.ops.set_workspace(ws)
        assert np.array_equal(c_percall, run_case(pk, "mx", a_bits, is_bf16, q, s, gs, m, n, k, native[0]))
        a_f32 = to_f32(a_bits, is_bf16)
        a_q = quantize_act_mxfp8(a_f32)
        dq = O.dequant_mxfp4(q, s)
        _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq, gs)               # same quantised activations
        _, full = O.gemm_ref(a_bits, is_bf16, dq, gs)                              # unquantised activations
        sum_abs = (np.abs(a_f32) @ np.abs(dq).T) * gs
        derived = native_exact_bound(a_q, dq, gs, "mxfp8")
        for sid in native:
            c = to_f32(run_case(pk, "mx", a_bits, is_bf16, q, s, gs, m, n, k, sid), is_bf16).astype(np.float64)
            fin = np.isfinite(full) & (np.abs(full) < (3e38 if is_bf16 else 6e4))
            # (1) the kernel computes exactly "MXFP8(activations) x MXFP4(weights)": only the accumulation inside and between the block-scaled MFMAs and
            #     the final 16-bit rounding separate it from the oracle -- bounded per output by native_exact_bound (derived from the instruction; rounds
            #     3-4 carried an empirical 1e-5 -> 2e-5 -> 4e-5 of sum|a||w| here, raised whenever a fuzz run found a worse element)
            err = np.abs(c - exact)[fin]
            assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)[fin]).all()
            native_p99_guard(err, exact[fin], ((np.abs(a_q) @ np.abs(dq).T) * gs)[fin], f"{sid:#x}")
            assert np.median(err / np.maximum(np.abs(exact[fin]), 1e-3)) < (2 ** -8 if is_bf16 else 2 ** -11) * 1.5   # (typical: one 16-bit rounding)
            # (2) stated tolerance of the path against the UNQUANTISED reference: e4m3 activations carry
            #     up to 2^-4 relative error each; on these random problems the result stays within 2 %
            #     of sum|a||w| (and typically ~3 % of the output's rms)
            assert (np.abs(c - full)[fin] <= 2e-2 * sum_abs[fin] + 1e-2).all()
            assert np.sqrt(np.mean((c - full)[fin] ** 2)) <= 6e-2 * np.sqrt(np.mean(full[fin] ** 2))
        # the fused SiLU-mul epilogue on the native kernels (even n-tiles per wave), against the exact-semantics oracle
        if n % 32 == 0 and fin.all() and np.abs(exact).max() < 50:
            gate, up = exact.astype(np.float64)[:, : n // 2], exact.astype(np.float64)[:, n // 2:]
            ref_act = gate / (1.0 + np.exp(-gate)) * up
            qd = torch.from_numpy(q).to(DEV)
            b = pk.repack_mxfp4(qd.view(torch.int32), n, k)
            sp = pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
            gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
            for sid in [x for x in native if ((x >> 52) & 0xF) % 2 == 0][:3]:
                c = pk.mul_mxfp4_a16(from_bits(a_bits, dtype).to(DEV), b, sp, gsd, m, n, k, sid, activation="silu_mul")
                cf = to_f32(bits(c), is_bf16).astype(np.float64)
                assert (np.abs(cf - ref_act) <= np.maximum(2e-2, 2e-2 * np.abs(ref_act))).all()
    finally:
        pk.ops.set_workspace(None)
        pk.ops.enable_native_fp4(False)


# --- NVFP4 weights on the native class (round 6): the MFMA-native image (csrc/nvnative.hip) and the WF = 6 kernels ----------------------

def _nv_checkpoint_like(n, k, seed):
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import quantize_weights as QW
    q, s, ws2 = QW.quantize_nvfp4(QW.synthetic_weights(n, k, seed=seed))
    return q, s, float(ws2)


@pytest.mark.parametrize("n,k,kind", [(32, 256, "uniform"), (48, 512, "uniform"), (272, 1024, "uniform"), (1024, 2048, "checkpoint"), (8192, 8192, "uniform")])
def test_nv6_image_device_equals_host(pk, n, k, kind):
    """petit_nvfp4_native_image (hardware convert v_cvt_scalef32_2xpk16_fp6_f32) and its host twin produce the same bytes -- negative scales, e4m3
    subnormal scales, zero blocks, N % 32 == 16 (half-empty last block) included -- and the bytes decode to oracle.nv6_reencode."""
    rng = np.random.default_rng(n * 3 + k)
    if kind == "uniform":
        q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
        s = rng.integers(0, 0x7F, (n, k // 16), dtype=np.uint8)
        s[rng.random(s.shape) < 0.05] |= 0x80
        q[rng.random((n, 1)).repeat(k // 2, axis=1) < 0.05] = 0          # whole zero rows (zero blocks)
    else:
        q, s, _ = _nv_checkpoint_like(n, k, n + k)
    qd = torch.from_numpy(q).to(DEV)
    b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
    sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    image = pk.nvfp4_native_image(b, sp, n, k)
    host = pk.offline.nvfp4_native_image_cpu(b.cpu(), sp.cpu(), n, k)
    dev_bytes = image.cpu()
    # (-0 elements: the sign of a zero product is the only bit the two may disagree on without changing a value; compare decoded values AND bytes)
    if not torch.equal(dev_bytes, host):
        d = pk.offline.nvfp4_native_image_dequant_cpu(dev_bytes, n, k).numpy()
        h = pk.offline.nvfp4_native_image_dequant_cpu(host, n, k).numpy()
        assert np.array_equal(d, h), "device and host images decode differently"
        diff = (dev_bytes != host).sum().item()
        raise AssertionError(f"{diff} image bytes differ although every decoded value agrees (sign of zero?)")
    if n * k <= 1 << 22:
        want, _ = O.nv6_reencode(q, s)
        assert np.array_equal(pk.offline.nvfp4_native_image_dequant_cpu(dev_bytes, n, k).numpy(), want)


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("m,n,k", [(64, 256, 1024), (130, 96, 2048), (512, 1024, 2048), (33, 64, 512), (5, 64, 1024), (1, 128, 768), (257, 176, 1280), (200, 512, 4096)])
def test_native_nvfp4_every_kernel(pk, m, n, k, is_bf16):
    """Every enumerated native kernel of the NVFP4 family (the three activation formats, K split 1 / 2), on ragged M, N % 32 == 16 and every span size:
    (1) exact semantics -- against the oracle run on the CPU-quantised activations and the image's weights (oracle.nv6_reencode) within the usual
    1e-2 bound / the bound derived from the instruction; (2) the class tolerance against the unquantised oracle on the TRUE NVFP4 weights: the
    activation class's bound plus the stated weight re-rounding bound."""
    a_bits, q, s, gs = random_problem("nv", m, n, k, 7171 + m + n + k, is_bf16)
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = dtype
    h.b_type = pk.DataType.float4_e2m1
    pk.ops.enable_native_fp4(False)
    assert all((sid >> 48) & 0xF != 13 for sid in pk.ops.get_fp4_solutions(h, m, n, k))   # opt-in only
    pk.ops.enable_native_fp4(True)
    try:
        native = [sid for sid in pk.ops.get_fp4_solutions(h, m, n, k) if (sid >> 48) & 0xF == 13]
        assert {(sid >> 32) & 7 for sid in native} == {2, 4, 6}
        qd = torch.from_numpy(q).to(DEV)
        b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
        sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
        image = pk.nvfp4_native_image(b, sp, n, k)
        gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
        ad = from_bits(a_bits, dtype).to(DEV)
        a_f32 = to_f32(a_bits, is_bf16)
        dq = O.dequant_nvfp4(q, s)
        dq6, sb = O.nv6_reencode(q, s)
        wb = np.maximum(2.0 ** -4 * np.abs(dq), np.repeat(np.ldexp(1.0, sb.astype(np.int64) - 127 - 4), 32, axis=1))
        _, full = O.gemm_ref(a_bits, is_bf16, dq, gs)
        sum_abs = (np.abs(a_f32) @ np.abs(dq).T) * gs
        w_term = (np.abs(a_f32) @ wb.T) * gs
        fin = np.isfinite(full) & (np.abs(full) < (3e38 if is_bf16 else 6e4))
        for code, quant, fmt, coef in ((2, quantize_act_mxfp8, "mxfp8", 2e-2), (4, quantize_act_mxfp6, "mxfp6", 2e-2), (6, quantize_act_mxfp4, "mxfp4", 0.12)):
            a_q = quant(a_f32)
            _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq6, gs)
            derived = native_exact_bound(a_q, dq6, gs, fmt)
            for sid in [x for x in native if (x >> 32) & 7 == code]:
                for splitk in (1, 2):
                    sk = (sid & ~(0xF << 60)) | (splitk << 60)
                    c = to_f32(bits(pk.mul_nvfp4_native(ad, image, gsd, m, n, k, sk)), is_bf16).astype(np.float64)
                    err = np.abs(c - exact)[fin]
                    assert (err <= np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)[fin]).all(), f"{sk:#x} max {err.max()}"
                    native_p99_guard(err, exact[fin], ((np.abs(a_q) @ np.abs(dq6).T) * gs)[fin], f"{sk:#x}")
                    assert np.median(err / np.maximum(np.abs(exact[fin]), 1e-3)) < (2 ** -8 if is_bf16 else 2 ** -11) * 1.5, f"{sk:#x}"
                    assert (np.abs(c - full)[fin] <= (coef * sum_abs + w_term)[fin] + 1e-2).all(), f"{sk:#x}"
            # pre-quantised activations (one launch) are bit-identical to quantising inside the call
            sid0 = [x for x in native if (x >> 32) & 7 == code][0]
            qa = pk.quantize_activations(ad, fmt)
            assert torch.equal(pk.mul_nvfp4_native(qa, image, gsd, m, n, k, sid0).view(torch.int16), pk.mul_nvfp4_native(ad, image, gsd, m, n, k, sid0).view(torch.int16))
        # the sentinels: through the class's own entry point, and -- once the image is attached -- through the reference's
        a_q = quantize_act_mxfp8(a_f32)
        _, exact = O.gemm_ref(O.f32_to_bf16_bits(a_q), True, dq6, gs)
        derived = native_exact_bound(a_q, dq6, gs, "mxfp8")
        bound = np.maximum(np.maximum(1e-2, 1e-2 * np.abs(exact)), derived)
        c1 = pk.mul_nvfp4_native(ad, image, gsd, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP8)
        assert (np.abs(to_f32(bits(c1), is_bf16) - exact)[fin] <= bound[fin]).all()
        exact_default = pk.mul_nvfp4_a16(ad, b, sp, gsd, m, n, k, -1)
        assert torch.equal(pk.mul_nvfp4_a16(ad, b, sp, gsd, m, n, k, -2), exact_default)       # nothing attached: the library default, as in the reference
        pk.attach_nvfp4_native(b, image)
        try:
            c2 = pk.mul_nvfp4_a16(ad, b, sp, gsd, m, n, k, -2)
            assert torch.equal(c2.view(torch.int16), c1.view(torch.int16))
            assert torch.equal(pk.mul_nvfp4_a16(ad, b, sp, gsd, m, n, k, -1), exact_default)   # -1 stays the exact class
        finally:
            pk.attach_nvfp4_native(b, None)
        assert torch.equal(pk.mul_nvfp4_a16(ad, b, sp, gsd, m, n, k, -2), exact_default)
        # fused SiLU-mul on the image (gate rows and up rows meet in one 32-row operand through the lanes' own addresses)
        if n % 32 == 0 and fin.all() and np.abs(exact).max() < 50:
            gate, up = exact.astype(np.float64)[:, : n // 2], exact.astype(np.float64)[:, n // 2:]
            ref_act = gate / (1.0 + np.exp(-gate)) * up
            for sid in [x for x in native if (x >> 32) & 7 == 2][:4]:
                cf = to_f32(bits(pk.mul_nvfp4_native(ad, image, gsd, m, n, k, sid, activation="silu_mul")), is_bf16).astype(np.float64)
                assert (np.abs(cf - ref_act) <= np.maximum(2e-2, 2e-2 * np.abs(ref_act))).all(), f"silu_mul {sid:#x}"
    finally:
        pk.ops.enable_native_fp4(False)


def test_native_nvfp4_through_the_c_abi_and_a_graph(pk):
    """petit_gemm_fp4_fp16_grid_ws with a native sentinel on NVFP4 weights: refused (PETIT_ERROR_KERNEL_SHAPE) without an image, runs on the attached
    image with per-call scratch, is capturable into a HIP graph, and petit_gemm_nvfp4_native gives the same bits."""
    from petit_kernel import _lib
    import ctypes as C
    m, n, k = 384, 512, 2048
    a_bits, q, s, gs = random_problem("nv", m, n, k, 99, True)
    b = pk.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k)
    image = pk.nvfp4_native_image(b, sp, n, k)
    ad = from_bits(a_bits, torch.bfloat16).to(DEV)
    gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    sid = C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6)
    need = int(_lib.lib.petit_gemm_workspace_bytes(C.byref(h), m, n, k, sid))
    assert need >= m * k * 3 // 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    c = torch.zeros((m, n), dtype=torch.bfloat16, device=DEV)

    def call(stream):
        return _lib.lib.petit_gemm_fp4_fp16_grid_ws(c.data_ptr(), ad.data_ptr(), b.data_ptr(), sp.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h), sid, None,
                                                    ws.data_ptr(), need, C.c_void_p(stream))
    cur = torch.cuda.current_stream().cuda_stream
    assert call(cur) == _lib.PETIT_ERROR_KERNEL_SHAPE and torch.count_nonzero(c) == 0
    pk.attach_nvfp4_native(b, image)
    try:
        assert call(cur) == 0
        want = pk.mul_nvfp4_native(ad, image, gsd, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP6)
        assert torch.equal(c.view(torch.int16), want.view(torch.int16))
        assert _lib.lib.petit_gemm_fp4_fp16_grid_ws(c.data_ptr(), ad.data_ptr(), b.data_ptr(), sp.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(h), sid, None,
                                                    None, 0, C.c_void_p(cur)) == _lib.PETIT_ERROR_KERNEL_SHAPE     # no scratch: refused, not another class
        c.zero_()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                assert call(st.cuda_stream) == 0
            g.replay()
            st.synchronize()
        assert torch.equal(c.view(torch.int16), want.view(torch.int16))
    finally:
        pk.attach_nvfp4_native(b, None)


def test_process_wide_default_class_runs_the_native_pick_behind_solution_id_minus_one(pk):
    """set_mxfp4_default_activations('mxfp6') (= $PETIT_AMD_MXFP4_ACTIVATIONS): an UNCHANGED call site -- mul_mxfp4_a16(..., -1), either binding --
    gets the MXFP6 class's default pick bit for bit at M >= 64, the exact kernel below that, on NVFP4 weights and through a C call without
    scratch; switching it off restores the exact default."""
    import ctypes as C
    from petit_kernel import _lib
    m, n, k = 192, 512, 2048
    a_bits, q, s, gs, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 8800)
    base = pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, -1)
    base16 = pk.mul_mxfp4_a16(a[:16].contiguous(), b, sp, gsd, 16, n, k, -1)
    assert pk.ops.mxfp4_default_activations() is None
    ch = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)

    def c_call_without_scratch():
        c = torch.empty_like(base)
        pk.ops.set_workspace(None)
        rc = _lib.lib.petit_gemm_mxfp4_fp16_grid(c.data_ptr(), a.data_ptr(), b.data_ptr(), sp.data_ptr(), gsd.data_ptr(), m, n, k, C.byref(ch),
                                                 C.c_uint64(_lib.PETIT_SOLUTION_AUTO), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        return c
    base_c = c_call_without_scratch()
    pk.ops.set_mxfp4_default_activations("mxfp6")
    try:
        want = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP6)
        assert not torch.equal(want.view(torch.int16), base.view(torch.int16))                      # (another accuracy class: it does differ)
        for use_compiled in (True, False):
            got = (pk.mul_mxfp4_a16 if use_compiled else pk.ops.mul_mxfp4_a16)(a, b, sp, gsd, m, n, k, -1)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(pk.mul_mxfp4_a16(a[:16].contiguous(), b, sp, gsd, 16, n, k, -1).view(torch.int16), base16.view(torch.int16))
        # the C entry point without any scratch: the exact default it ran before (a kernel that needs none), not an error
        assert torch.equal(c_call_without_scratch().view(torch.int16), base_c.view(torch.int16))
        # NVFP4 weights are not affected
        an, qn, sn, gn = random_problem("nv", m, n, k, 8801, True)
        check_gemm(run_case(pk, "nv", an, True, qn, sn, gn, m, n, k), oracle_ref("nv", an, True, qn, sn, gn), True, None)
    finally:
        pk.ops.set_mxfp4_default_activations(None)
    assert torch.equal(pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, -1).view(torch.int16), base.view(torch.int16))


# --- tune-and-persist inside the library (csrc/tune.hip; the reference's `bench_matmul -algo tune`, main.cc:269-325) ------

def test_in_library_tune_picks_checks_and_persists(pk, tmp_path):
    """petit_kernel.tune_tensors on shapes no table knows: the winner is an enumerated kernel (possibly with a K split), it
    becomes what solution_id = -1 resolves to for its M bucket at once, the AUTO output still matches the oracle, the class
    sentinel -3 follows a native-class tune, and the saved file reproduces the pick in a fresh process."""
    import os
    import subprocess
    import sys
    from petit_kernel import _lib
    for kind, m, n, k in (("nv", 16, 2048, 4096), ("nv", 200, 256, 16384), ("mx", 40, 1024, 2048)):
        a_bits, q, s, gs = random_problem(kind, m, n, k, 4400 + m, True)
        a = from_bits(a_bits, torch.bfloat16).to(DEV)
        qd = torch.from_numpy(q).to(DEV)
        gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
        b = pk.repack_nvfp4(qd.view(torch.int32), n, k)
        sp = (pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k) if kind == "nv"
              else pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k))
        h = pk.PetitSolutionHints()
        h.a_type = h.c_type = torch.bfloat16
        h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
        sid, us = pk.tune_tensors(a, (b, sp), gsd, m, n, k, kind="nvfp4" if kind == "nv" else "mxfp4", rotate_mb=96)
        assert us > 0 and (sid & ~(0xF << 60)) | (1 << 60) in pk.ops.get_fp4_solutions(h, m, n, k)
        assert pk.ops.resolve_solution(h, m, n, k, -1) == sid
        c = (pk.mul_nvfp4_a16 if kind == "nv" else pk.mul_mxfp4_a16)(a, b, sp, gsd, m, n, k, -1)
        check_gemm(bits(c), oracle_ref(kind, a_bits, True, q, s, gs), True, oracle_sum_abs(kind, a_bits, True, q, s, gs))
        if kind == "mx":
            nsid, nus = pk.tune_tensors(a, (b, sp), gsd, m, n, k, kind="mxfp4", klass="native_mxfp4", rotate_mb=96)
            assert (nsid >> 48) & 0xF == 13 and (nsid >> 32) & 7 == 6 and nus > 0
            assert pk.ops.resolve_solution(h, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP4) == nsid
            assert pk.ops.resolve_solution(h, m, n, k, -1) == sid          # the exact class is untouched by it
            n6, us6 = pk.tune_tensors(a, (b, sp), gsd, m, n, k, kind="mxfp4", klass="native_mxfp6", rotate_mb=96)
            assert (n6 >> 48) & 0xF == 13 and (n6 >> 32) & 7 == 4 and us6 > 0
            assert pk.ops.resolve_solution(h, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP6) == n6
            assert pk.ops.resolve_solution(h, m, n, k, pk.SOLUTION_AUTO_NATIVE_MXFP4) == nsid   # each class keeps its own row
    path = tmp_path / "tuned.txt"
    pk.tuning.save(path)
    rows = [ln.split() for ln in path.read_text().splitlines() if ln and not ln.startswith("#")]
    assert len(rows) >= 4
    at, bt, n, k, lo, hi, sol = rows[-1]     # the oldest row: the first problem tuned above
    code = ("import sys, ctypes as C; sys.path.insert(0, r'%s'); from petit_kernel import _lib; h = _lib.SolutionHints(%s, %s, %s, 0); "
            "print('%%x' %% _lib.lib.petit_gemm_default_solution(C.byref(h), %s, %s, %s))" % (ROOT / "petit-kernel_amd", at, bt, at, lo, n, k))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PETIT_AMD_TUNE_FILE=str(path)), capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == sol


def test_inlib_tune_ranks_large_m_kernels_on_wide_range_mx_outputs(pk):
    """Regression (round 3): the tuner compared a candidate with its reference kernel as |c - ref| <= tol * max(1, |ref|).  On a long K with
    MXFP4 block scales up to 2^8 the outputs have an rms of ~1e4 and elements where the terms cancel differ by ~1 between two exact kernels'
    summation orders: every tiled / 32x32 kernel was rejected and a streaming kernel 2-5x slower won (tools/refresh_table.py flagged this very
    problem: fp16 x MXFP4, 4096 x 14336, M = 128: default 35 us, the old tuner's pick 66 us).  The floor is the output's rms now: the tuner's pick,
    timed the way the refresh tool times it, must not be slower than what solution_id = -1 runs."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import benchlib as BL
    m, n, k = 128, 4096, 14336
    w = BL.Weights("mx", n, k, 256, DEV)
    g = BL.Gemm(w, m, torch.float16, DEV)
    stream = torch.cuda.Stream(DEV)
    dflt = g.resolve(pk.ops._lib.PETIT_SOLUTION_AUTO)
    with torch.cuda.stream(stream):
        sid, _ = pk.tune_tensors(g.a, w.packed, g.gs, m, n, k, "mxfp4", persist=False)
    t_dflt, t_pick = g.time(dflt, stream, reps=3)["us"], g.time(sid, stream, reps=3)["us"]
    assert t_pick <= 1.25 * t_dflt, (pk.ops._lib.describe_solution(sid), t_pick, t_dflt)


def test_autotune_on_first_sight(pk, tmp_path):
    """$PETIT_AMD_AUTOTUNE=1 + $PETIT_AMD_TUNE_FILE: the first solution_id = -1 call of an unseen shape tunes it in place (the call's own
    scratch, clones of the caller's weights out of the reserved pool), returns the right result, and leaves a row in the file; the second
    call and a graph capture run without tuning again; a first-sight tune on one stream while ANOTHER stream is inside torch.cuda.graph
    leaves that capture intact (the run exchanges the thread's capture mode to relaxed: tools/probes/capture_legal.hip), without a reserved
    pool (hipMalloc) and with one; rows another process saved meanwhile survive the save."""
    import os
    import subprocess
    import sys
    path = tmp_path / "auto_tuned.txt"
    code = r"""
import sys
sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s')
import numpy as np, torch
import petit_kernel as pk
from petit_kernel import _lib
m, n, k = 12, 1536, 3072
g = torch.Generator().manual_seed(5)
a = torch.randn((m, k), generator=g).bfloat16().cuda()
q = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8).cuda()
s = (torch.rand((n, k // 16), generator=g) * 3.5 + 0.25).to(torch.float8_e4m3fn).cuda()
gs = torch.tensor([1.0], device='cuda')
b = pk.repack_nvfp4(q.view(torch.int32), n, k); sp = pk.process_nvfp4_scales(s, n, k)
h = pk.PetitSolutionHints(); h.a_type = h.c_type = torch.bfloat16; h.b_type = pk.DataType.float4_e2m1
g0 = _lib.lib.petit_tune_generation()
c1 = pk.mul_nvfp4_a16(a, b, sp, gs, m, n, k, -1)
assert _lib.lib.petit_tune_generation() == g0 + 1, 'first sight must tune'
picked = pk.ops.resolve_solution(h, m, n, k, -1)
c2 = pk.mul_nvfp4_a16(a, b, sp, gs, m, n, k, picked)
assert torch.equal(c1.view(torch.int16), c2.view(torch.int16))
dense = pk.ops.dequant_packed(b, sp, n, k, 'nvfp4')
ref = a.float() @ dense.t()
assert torch.allclose(c1.float(), ref, rtol=1e-2, atol=1e-2 * ref.abs().max().item())
pk.mul_nvfp4_a16(a, b, sp, gs, m, n, k, -1)
assert _lib.lib.petit_tune_generation() == g0 + 1, 'second call must not tune again'
a9 = a[:9].contiguous()
pk.mul_nvfp4_a16(a9, b, sp, gs, 9, n, k, -1)
assert _lib.lib.petit_tune_generation() == g0 + 1, 'same M bucket: the row serves it'
gr = torch.cuda.CUDAGraph()
with torch.cuda.graph(gr):
    pk.mul_nvfp4_a16(a9, b, sp, gs, 9, n, k, -1)      # same M bucket (9..16): served by the row, nothing to tune under capture
gr.replay(); torch.cuda.synchronize()
# --- a first-sight tune while another stream is being captured (global capture mode: what torch.cuda.graph uses).  Through the C ABI with
# preallocated output and scratch: torch's own allocator calls a plain hipMalloc for an allocation on a stream that is not the capturing
# one (and torch.cuda.graph empties its cache on entry), which breaks the capture before the library is even called.
import ctypes as C
def c_abi_call(a_, c_, ws_, m_):
    hh = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    rc = _lib.lib.petit_gemm_fp4_fp16_grid_ws(C.c_void_p(c_.data_ptr()), C.c_void_p(a_.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(sp.data_ptr()),
                                              C.c_void_p(gs.data_ptr()), m_, n, k, C.byref(hh), C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None,
                                              C.c_void_p(ws_.data_ptr()), C.c_uint64(ws_.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
side, other = torch.cuda.Stream(), torch.cuda.Stream()
x = torch.ones(4096, device='cuda')
for m2, reserve_mb in ((40, 0), (100, 512)):      # M buckets 33..48 and 65..128: unseen; without and with a reserved pool (petit_tune_reserve)
    a2 = torch.randn((m2, k), generator=g).bfloat16().cuda()
    c2_ = torch.empty((m2, n), dtype=torch.bfloat16, device='cuda')
    ws2 = torch.empty(32 << 20, dtype=torch.uint8, device='cuda')
    if reserve_mb:
        pk.tuning.reserve(reserve_mb)
    gen_before = _lib.lib.petit_tune_generation()
    other.wait_stream(torch.cuda.current_stream()); torch.cuda.synchronize()
    gr2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr2, stream=side):
        y = x * 2 + 1
        with torch.cuda.stream(other):         # not the capturing stream
            c_abi_call(a2, c2_, ws2, m2)
        z = y * 3
    assert _lib.lib.petit_tune_generation() == gen_before + 1, 'the unseen bucket must have been tuned during the capture'
    other.synchronize()
    ref2 = a2.float() @ dense.t()
    assert torch.allclose(c2_.float(), ref2, rtol=1e-2, atol=1e-2 * ref2.abs().max().item())
    x.fill_(2.0); gr2.replay(); torch.cuda.synchronize()
    assert torch.equal(z, torch.full_like(z, 15.0)), 'the capture on the other stream must have survived the tune'
    x.fill_(1.0)
pk.tuning.reserve(0)
print('%%x' %% picked)
""" % (ROOT / "petit-kernel_amd", ROOT)
    path.write_text("# saved by another process\n5 3 777 1024 1 1 abc\n")
    env = dict(os.environ, PETIT_AMD_AUTOTUNE="1", PETIT_AMD_TUNE_FILE=str(path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    picked = out.stdout.strip().splitlines()[-1]
    rows = [ln.split() for ln in path.read_text().splitlines() if ln and not ln.startswith("#")]
    assert {tuple(r[:6]) for r in rows} >= {("5", "3", "1536", "3072", "9", "16"), ("5", "3", "1536", "3072", "33", "48"), ("5", "3", "1536", "3072", "65", "128")}   # (M = 40: the 33-48 sub-bucket of round 6)
    assert [r[6] for r in rows if r[4] == "9"] == [picked]
    assert ["5", "3", "777", "1024", "1", "1", "abc"] in rows, "a row another process saved must survive this process's save"


# --- the native class as a pipeline: pre-quantised activations in, quantised SiLU-mul out (petit_gemm_mxfp4_native) --------

def decode_qact(raw: np.ndarray, m: int, k: int, fmt: str) -> np.ndarray:
    """'petit-qact/1' bytes -> the dequantised [m, k] activations (csrc/gemm_native32.hpp, workspace layout note): data
    [K/128][M][16 ACT bytes] then scales [K/128][M][4] E8M0 bytes; FP4: natural nibble order; FP8: the eight 16-column units of a
    tile sit at positions (u & 4) | ((u & 1) << 1) | ((u >> 1) & 1)."""
    act = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}[fmt]
    kt = k // 128
    sc = raw[m * k // 8 * act:].reshape(kt, m, 4).astype(np.int32)
    scale = np.ldexp(1.0, sc - 127)                                      # [kt][m][4 blocks of 32]
    if act == 6:
        # two images: registers 0-3 of block b at byte 16 b of a 64-byte row, registers 4-5 of blocks 0, 2, 1, 3 in a 32-byte row;
        # element i of a block at bits [6 i, 6 i + 6) of its 24 bytes
        lo = raw[: m * k // 2].reshape(kt, m, 4, 16)
        hi = raw[m * k // 2: m * k // 8 * 6].reshape(kt, m, 4, 8)[:, :, [0, 2, 1, 3], :]
        blocks = np.concatenate([lo, hi], axis=-1)                                   # [kt][m][4][24 bytes]
        bits_ = np.unpackbits(blocks, axis=-1, bitorder="little").reshape(kt, m, 4, 32, 6)
        codes = (bits_ * (1 << np.arange(6))).sum(axis=-1)
        vals = np.where(codes & 32, -1.0, 1.0) * E2M3_GRID[codes & 31]
        out = vals * scale[..., None]
        return out.reshape(kt, m, 128).transpose(1, 0, 2).reshape(m, k).astype(np.float32)
    data = raw[: m * k // 8 * act].reshape(kt, m, 16 * act)
    if act == 4:
        lo, hi = data & 0xF, data >> 4
        codes = np.stack([lo, hi], axis=-1).reshape(kt, m, 128)
        vals = O.FP4_VALUES[codes]
    else:
        vals8 = torch.from_numpy(data.copy()).view(torch.float8_e4m3fn).float().numpy().reshape(kt, m, 8, 16)
        pos = [(u & 4) | ((u & 1) << 1) | ((u >> 1) & 1) for u in range(8)]
        vals = vals8[:, :, pos, :].reshape(kt, m, 128)
    out = vals.reshape(kt, m, 4, 32) * scale[..., None]
    return out.reshape(kt, m, 128).transpose(1, 0, 2).reshape(m, k).astype(np.float32)


def NATIVE_SENTINEL(pk, fmt):
    return {"mxfp8": pk.SOLUTION_AUTO_NATIVE_MXFP8, "mxfp6": pk.SOLUTION_AUTO_NATIVE_MXFP6, "mxfp4": pk.SOLUTION_AUTO_NATIVE_MXFP4}[fmt]


def _mx_problem_on_device(pk, m, n, k, seed, dtype=torch.bfloat16):
    a_bits, q, s, gs = random_problem("mx", m, n, k, seed, dtype == torch.bfloat16)
    a = from_bits(a_bits, dtype).to(DEV)
    b = pk.repack_mxfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
    sp = pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k)
    return a_bits, q, s, gs, a, b, sp, torch.tensor([gs], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("fmt,code", [("mxfp8", 2), ("mxfp6", 4), ("mxfp4", 6)])
@pytest.mark.parametrize("m,n,k", [(64, 256, 1024), (130, 96, 2048), (512, 1024, 2048), (33, 64, 512), (1, 128, 768)])
def test_prequantized_activations_equal_on_the_fly(pk, m, n, k, fmt, code):
    """quantize_activations() once + the GEMM on the quantised bytes (ONE launch) is bit-identical to the two-launch call on
    the 16-bit activations, for every 32x32x64 kernel of the format, the class sentinel and a K split; the decoded bytes are
    exactly the CPU statement of the quantiser; a 16x16x128 kernel (other operand order) and a format mismatch are refused."""
    a_bits, q, s, gs, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 6100 + m + n + k)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.mxfloat4_e2m1
    qa = pk.quantize_activations(a, fmt)
    want = {"mxfp8": quantize_act_mxfp8, "mxfp6": quantize_act_mxfp6, "mxfp4": quantize_act_mxfp4}[fmt](to_f32(a_bits, True))
    assert np.array_equal(decode_qact(qa.data.cpu().numpy(), m, k, fmt), want)
    pk.ops.enable_native_fp4(True)
    try:
        sols = pk.ops.get_fp4_solutions(h, m, n, k)
        k32 = [x for x in sols if (x >> 48) & 0xF == 13 and (x >> 32) & 7 == code]
        assert k32
        sentinel = NATIVE_SENTINEL(pk, fmt)
        for sid in k32 + [(k32[0] & ~(0xF << 60)) | (2 << 60), sentinel]:
            two = pk.mul_mxfp4_a16(a, b, sp, gsd, m, n, k, sid) if sid != sentinel else None
            one = pk.mul_mxfp4_native(qa, b, sp, gsd, m, n, k, sid)
            if two is None:      # the sentinel may resolve to a 16x16x128 kernel for 16-bit input; with quantised input it must be a 32x32x64 one
                two = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, k32[0])
                assert check_gemm(bits(one), to_f32(bits(two), True), True) is None
            else:
                assert torch.equal(one.view(torch.int16), two.view(torch.int16)), hex(sid)
        k16 = [x for x in sols if (x >> 48) & 0xF == 9]
        if k16 and fmt == "mxfp8":
            with pytest.raises(RuntimeError):
                pk.mul_mxfp4_native(qa, b, sp, gsd, m, n, k, k16[0])
        other = pk.SOLUTION_AUTO_NATIVE_MXFP4 if fmt != "mxfp4" else pk.SOLUTION_AUTO_NATIVE_MXFP8
        with pytest.raises(RuntimeError):
            pk.mul_mxfp4_native(qa, b, sp, gsd, m, n, k, other)
        with pytest.raises(RuntimeError):
            pk.mul_mxfp4_native(qa, b, sp, gsd, m, n, k, -1)           # plain AUTO never runs the native class
    finally:
        pk.ops.enable_native_fp4(False)


@pytest.mark.parametrize("is_bf16", [True, False])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_activation_quantiser_on_hostile_blocks(pk, fmt, is_bf16):
    """petit_quantize_activations against its CPU statement on blocks chosen to hit every branch of the rounding: all-zero blocks (scale byte 127),
    -0.0, one huge value next to tiny ones (everything else flushes or lands in the subnormals), block maxima just below / at / above the
    saturation point of the element format, exact ties between two codes (round to even), values one ulp either side of a tie, negative twins of
    all of them, 16-bit subnormals, and blocks whose exponent sits at the ends of the 16-bit type's range."""
    rng = np.random.default_rng(99)
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    m, k = 16, 2048
    a = rng.standard_normal((m, k)).astype(np.float32)
    grid = {"mxfp8": None, "mxfp6": E2M3_GRID, "mxfp4": E2M1_GRID}[fmt]
    blocks = a.reshape(m, k // 32, 32)
    blocks[0, 0] = 0.0
    blocks[0, 1] = -0.0
    blocks[0, 2, :] = 1e-3
    blocks[0, 2, 5] = 3.0e4 if is_bf16 else 3.0e3                       # one outlier: the rest of the block is far below a code
    top = 7.5 if fmt == "mxfp6" else 6.0 if fmt == "mxfp4" else 7.0
    for j, mx in enumerate((top * 0.999, top, top * 1.03, 7.99, 4.0, 3.999)):   # block maxima around the saturation point (block scale 2^0 .. )
        blocks[1, j] = rng.uniform(-1, 1, 32)
        blocks[1, j, 7] = mx
        blocks[2, j] = -blocks[1, j]
    if grid is not None:                                                # exact ties and their neighbours, at two block scales
        mids = (grid[:-1] + grid[1:]) / 2
        for j, sc in enumerate((1.0, 2.0 ** -9 if not is_bf16 else 2.0 ** -40, 2.0 ** 7)):
            vals = np.concatenate([mids, mids * (1 + 2.0 ** -7), mids * (1 - 2.0 ** -7)])[:31]
            blocks[3, j, :31] = 0.0
            blocks[3, j, :len(vals)] = vals * sc
            blocks[3, j, 31] = 7.0 * sc                                 # pins the block's scale: maximum in [4, 8) * sc
            blocks[4, j] = -blocks[3, j]
    tiny = 2.0 ** -133 if is_bf16 else 2.0 ** -24                       # subnormals of the 16-bit type
    blocks[5, 0] = tiny * rng.integers(0, 8, 32)
    blocks[5, 1] = rng.standard_normal(32) * (2.0 ** 120 if is_bf16 else 2.0 ** 14)
    a = blocks.reshape(m, k)
    a_bits = O.f32_to_bf16_bits(a) if is_bf16 else a.astype(np.float16).view(np.uint16)
    x = to_f32(a_bits, is_bf16)
    want = {"mxfp8": quantize_act_mxfp8, "mxfp6": quantize_act_mxfp6, "mxfp4": quantize_act_mxfp4}[fmt](x)
    qa = pk.quantize_activations(from_bits(a_bits, dtype).to(DEV), fmt)
    got = decode_qact(qa.data.cpu().numpy(), m, k, fmt)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ; first: row {bad[0][0]} col {bad[0][1]}: x {x[tuple(bad[0])]!r} got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
@pytest.mark.parametrize("m,n,k,with_bias", [(64, 512, 1024, False), (130, 1024, 512, True), (512, 1536, 2048, False), (5, 512, 768, False)])
def test_quantized_silu_mul_output_feeds_the_next_gemm(pk, m, n, k, with_bias, fmt):
    """gate_up with the quantising SiLU-mul epilogue (out_quantized): the emitted bytes decode to the 16-bit fused result within
    one quantisation step of their block (scale byte = the quantiser's rule on the block maximum), and `down` run on them equals
    `down` run on quantize_activations(16-bit result) up to the double rounding the fused form avoids."""
    a_bits, q, s, gs, a, b, sp, gsd = _mx_problem_on_device(pk, m, n, k, 7300 + m + n + k)
    bias = (torch.randn(n, device=DEV) * 0.5).bfloat16() if with_bias else None
    sentinel = NATIVE_SENTINEL(pk, fmt)
    h = pk.PetitSolutionHints()
    h.a_type = h.c_type = torch.bfloat16
    h.b_type = pk.DataType.mxfloat4_e2m1
    c16 = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, bias=bias, activation="silu_mul")
    qout = pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, bias=bias, activation="silu_mul", out_quantized=fmt)
    assert isinstance(qout, pk.QuantizedActivations) and (qout.m, qout.k, qout.fmt) == (m, n // 2, fmt)
    ref16 = c16.float().cpu().numpy()
    deq = decode_qact(qout.data.cpu().numpy(), m, n // 2, fmt)
    blk = np.abs(ref16).reshape(m, -1, 32).max(axis=2)
    step = np.repeat(np.exp2(np.floor(np.log2(np.maximum(blk, 1e-30)))), 32, axis=1).reshape(m, -1)   # 2^E of the block maximum
    err = np.abs(deq - ref16)
    if fmt == "mxfp4":      # e2m1 on [0, 8) 2^(E-2): spacing <= 2^(E-1), saturation of (6, 8) costs up to 2^(E-1) more
        assert (err <= 0.5 * step + 2.0 ** -7 * np.abs(ref16)).all(), err.max()
    elif fmt == "mxfp6":    # e2m3 on [0, 8) 2^(E-2): half a spacing is <= 2^-4 relative (normals) or 2^(E-6) (subnormals); (7.5, 8) clips by <= 2^(E-3)
        assert (err <= 2.0 ** -4 * np.abs(ref16) + 2.0 ** -6 * step + 2.0 ** -7 * np.abs(ref16) + np.where(np.abs(ref16) > 1.875 * step, 0.125 * step, 0.0)).all(), err.max()
    else:                   # e4m3: 2^-4 relative, block maximum mapped into [128, 256) (never saturates)
        assert (err <= 2.0 ** -4 * np.abs(ref16) + 2.0 ** -9 * step + 2.0 ** -7 * np.abs(ref16)).all(), err.max()
    # (measured: mxfp8 2.6 %, mxfp6 3.1 % -- the same three mantissa bits, plus subnormals from 1/8 of the block maximum down -- mxfp4 11 %)
    assert np.sqrt(np.mean(err ** 2)) <= {"mxfp4": 0.15, "mxfp6": 0.04, "mxfp8": 0.03}[fmt] * np.sqrt(np.mean(ref16 ** 2))
    # the consumer: down = [n2, n / 2] MXFP4 weights
    n2 = 256
    _, q2, s2, gs2 = random_problem("mx", 1, n2, n // 2, 99 + n, True)
    b2 = pk.repack_mxfp4(torch.from_numpy(q2).to(DEV).view(torch.int32), n2, n // 2)
    sp2 = pk.process_mxfp4_scales(torch.from_numpy(s2).to(DEV), n2, n // 2)
    gsd2 = torch.tensor([gs2], dtype=torch.float32, device=DEV)
    y_fused = pk.mul_mxfp4_native(qout, b2, sp2, gsd2, m, n2, n // 2, sentinel).float()
    y_two = pk.mul_mxfp4_native(pk.quantize_activations(c16, fmt), b2, sp2, gsd2, m, n2, n // 2, sentinel).float()
    diff = (y_fused - y_two).pow(2).mean().sqrt().item() / max(y_two.pow(2).mean().sqrt().item(), 1e-9)
    assert diff <= {"mxfp4": 0.08, "mxfp6": 0.03, "mxfp8": 0.02}[fmt], diff
    # and it really is the dequantised bytes that were multiplied: the oracle on `deq`
    dq2 = O.dequant_mxfp4(q2, s2)
    _, want = O.gemm_ref(O.f32_to_bf16_bits(deq), True, dq2, gs2)
    check_gemm(bits(pk.mul_mxfp4_native(qout, b2, sp2, gsd2, m, n2, n // 2, sentinel)), want, True,
               (np.abs(deq) @ np.abs(dq2).T) * gs2, sum_abs_coef=1e-4)      # (silu(g) * u of e8m0-scaled weights: terms of 1e12 cancelling)
    # what the entry point refuses
    pk.ops.enable_native_fp4(True)
    try:
        small = next(x for x in pk.ops.get_fp4_solutions(h, m, n, k) if (x >> 48) & 0xF == 13 and (x >> 52) & 0xF == 2)
        with pytest.raises(RuntimeError):
            pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, small, activation="silu_mul", out_quantized=fmt)   # 128-column tiles
    finally:
        pk.ops.enable_native_fp4(False)
    with pytest.raises(RuntimeError):
        pk.mul_mxfp4_native(a, b, sp, gsd, m, n, k, sentinel, out_quantized=fmt)                             # no SiLU-mul


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6", "mxfp4"])
def test_native_silu_mul_with_activation_only_scratch_writes_its_output(pk, fmt):
    """AUTO_NATIVE_* + SiLU-mul on N = 1280, K = 8192, M = 512, where the native table names the 64 x 320 kernel (five n-tiles per
    wave) with a K split of 4 / 8 -- fine while the reduce pass applies the activation.  With scratch that covers the quantised activations ONLY
    (petit_native_workspace_bytes) the library used to drop the split, keep the kernel, and return PETIT_OK with C unwritten (that kernel's own
    SiLU-mul epilogue exists for even n-tile counts only).  Now: the call re-picks a kernel that applies SiLU-mul itself; the output equals, within the
    class tolerance, what the full-scratch call computes -- and a poison pattern in C is gone."""
    import ctypes as C
    from petit_kernel import _lib
    m, n, k = 512, 1280, 8192
    _, _, _, _, a, b, sp, gs = _mx_problem_on_device(pk, m, n, k, 77)
    sid = NATIVE_SENTINEL(pk, fmt)
    full = pk.mul_mxfp4_native(a, b, sp, gs, m, n, k, sid, activation="silu_mul")
    torch.cuda.synchronize()
    assert full.shape == (m, n // 2) and torch.isfinite(full.float()).all()
    hints = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    epi = _lib.Epilogue(None, 1, 0)
    need = int(_lib.lib.petit_native_workspace_bytes(m, k))
    picked = int(_lib.lib.petit_gemm_resolve_solution(C.byref(hints), m, n, k, C.c_uint64(sid & (2 ** 64 - 1)), C.byref(epi), C.c_uint64(need)))
    assert picked and picked >> 60 == 1 and ((picked >> 52) & 0xF) % 2 == 0, hex(picked)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    c = torch.full((m, n // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = _lib.lib.petit_gemm_mxfp4_native(C.c_void_p(c.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(sp.data_ptr()),
                                          C.c_void_p(gs.data_ptr()), m, n, k, C.byref(hints), C.c_uint64(sid & (2 ** 64 - 1)), C.byref(epi), None,
                                          C.c_void_p(ws.data_ptr()), C.c_uint64(need), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert torch.isfinite(c.float()).all(), "the output buffer was not (fully) written"
    rms = full.float().pow(2).mean().sqrt().item()
    rel = (c.float() - full.float()).pow(2).mean().sqrt().item() / rms
    assert rel <= 2e-2, rel      # same quantised activations, same weights: only the summation order and one bf16 rounding differ
    # an explicit id of the odd-n-tile kernel with SiLU-mul and no split is refused, never a silent no-op
    pk.ops.enable_native_fp4(True)
    try:
        h = pk.PetitSolutionHints()
        h.a_type = h.c_type = torch.bfloat16
        h.b_type = pk.DataType.mxfloat4_e2m1
        odd = [s_ for s_ in pk.ops.get_fp4_solutions(h, m, n, k) if (s_ >> 48) & 0xF in (9, 13) and ((s_ >> 52) & 0xF) % 2 == 1]
        assert odd
        for s_ in odd[:3]:
            with pytest.raises(RuntimeError):
                pk.mul_mxfp4_native(a, b, sp, gs, m, n, k, s_, activation="silu_mul")
    finally:
        pk.ops.enable_native_fp4(False)


def test_mlp_block_accuracy_budget(pk):
    """SURVEY.md section 8 f3 / the reference's model-level claim (README.md:3): an accuracy budget for the native class beyond
    one GEMM.  A synthetic gated-MLP block x -> gate_up -> SiLU-mul -> down (hidden 2048, intermediate 4096, MXFP4 weights,
    M = 96 tokens) with OUTLIER CHANNELS in x (six input columns x 60, the shape LLM activations have), three ways:
      exact  : the default kernels (bf16 activations end to end, fused SiLU-mul),
      mxfp8  : the native pipeline, activations quantised to MXFP8 at both GEMMs (quantiser + 2 launches),
      mxfp4  : the same with MXFP4 activations,
    each against the f64 oracle of the block.  Errors are reported relative to the rms of the block's output and bounded with
    margin over what MI355X measured."""
    import json
    hid, inter, m = 2048, 4096, 96
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((m, hid), dtype=np.float32)
    x[:, rng.choice(hid, 6, replace=False)] *= 60.0
    x_bits = O.f32_to_bf16_bits(x)
    _, q1, s1, _ = random_problem("mx", 1, 2 * inter, hid, 11, True, mx_band=(122, 127))
    _, q2, s2, _ = random_problem("mx", 1, hid, inter, 12, True, mx_band=(122, 127))
    gs1, gs2 = 0.05, 0.05
    dq1, dq2 = O.dequant_mxfp4(q1, s1).astype(np.float64), O.dequant_mxfp4(q2, s2).astype(np.float64)
    xf = to_f32(x_bits, True).astype(np.float64)
    y1 = xf @ dq1.T * gs1
    act = y1[:, :inter] / (1.0 + np.exp(-y1[:, :inter])) * y1[:, inter:]
    ref = act @ dq2.T * gs2
    rms = np.sqrt(np.mean(ref ** 2))
    xd = from_bits(x_bits, torch.bfloat16).to(DEV)
    b1 = pk.repack_mxfp4(torch.from_numpy(q1).to(DEV).view(torch.int32), 2 * inter, hid)
    sp1 = pk.process_mxfp4_scales(torch.from_numpy(s1).to(DEV), 2 * inter, hid)
    b2 = pk.repack_mxfp4(torch.from_numpy(q2).to(DEV).view(torch.int32), hid, inter)
    sp2 = pk.process_mxfp4_scales(torch.from_numpy(s2).to(DEV), hid, inter)
    g1, g2 = torch.tensor([gs1], device=DEV), torch.tensor([gs2], device=DEV)
    out = {}
    h1 = pk.mul_mxfp4_a16(xd, b1, sp1, g1, m, 2 * inter, hid, -1, activation="silu_mul")
    out["exact"] = pk.mul_mxfp4_a16(h1, b2, sp2, g2, m, hid, inter, -1)
    for fmt, sid in (("mxfp8", pk.SOLUTION_AUTO_NATIVE_MXFP8), ("mxfp6", pk.SOLUTION_AUTO_NATIVE_MXFP6), ("mxfp4", pk.SOLUTION_AUTO_NATIVE_MXFP4)):
        hq = pk.mul_mxfp4_native(pk.quantize_activations(xd, fmt), b1, sp1, g1, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=fmt)
        out[fmt] = pk.mul_mxfp4_native(hq, b2, sp2, g2, m, hid, inter, sid)
    report = {}
    for name, y in out.items():
        e = y.float().cpu().numpy().astype(np.float64) - ref
        report[name] = {"rms_err_over_rms": float(np.sqrt(np.mean(e ** 2)) / rms), "max_err_over_rms": float(np.abs(e).max() / rms)}
    print("mlp block accuracy budget:", json.dumps(report))
    dump = ROOT / "gpurun_out"
    if dump.is_dir():
        (dump / "mlp_accuracy_budget.json").write_text(json.dumps({"hidden": hid, "intermediate": inter, "m": m, "outlier_columns": 6,
                                                                   "outlier_factor": 60, "errors_relative_to_output_rms": report}, indent=1))
    assert report["exact"]["rms_err_over_rms"] <= 1e-2
    assert report["mxfp8"]["rms_err_over_rms"] <= 8e-2
    assert report["mxfp6"]["rms_err_over_rms"] <= 0.11       # (e4m3's three mantissa bits, but only three binades of them: next to an outlier x 60 the rest of a block is subnormal)
    assert report["mxfp4"]["rms_err_over_rms"] <= 0.45


# --- grouped launch: several weight matrices sharing the activation rows in one launch (petit_gemm_fp4_fp16_grouped) ---------

@pytest.mark.parametrize("m", [1, 3, 8, 16])
@pytest.mark.parametrize("kind,is_bf16", [("nv", True), ("nv", False), ("mx", True), ("mx", False)])
def test_grouped_launch(pk, kind, is_bf16, m):
    """Members of different N (ragged n-tile counts, one with a bias) against the oracle through solution_id = -1, and, for EVERY
    kernel that has a grouped form, bit-identical to separate calls with the same id; what the entry point refuses.  Includes the
    bench cell's shape (three 1280 x 8192 shards, tools/benchlib.py GroupedGemm)."""
    dtype = torch.bfloat16 if is_bf16 else torch.float16
    name = "nvfp4" if kind == "nv" else "mxfp4"
    for k, ns in ((2048, [256, 96 if kind == "nv" else 64, 1056]), (8192, [1280, 1280, 1280])):
        a_bits = random_problem(kind, m, 32, k, 900 + m, is_bf16)[0]
        a = from_bits(a_bits, dtype).to(DEV)
        members, refs = [], []
        for i, n in enumerate(ns):
            _, q, s, gs = random_problem(kind, 1, n, k, 910 + 7 * i + n, is_bf16)
            b = pk.repack_nvfp4(torch.from_numpy(q).to(DEV).view(torch.int32), n, k)
            sp = (pk.process_nvfp4_scales(torch.from_numpy(s).to(DEV).view(torch.float8_e4m3fn), n, k) if kind == "nv"
                  else pk.process_mxfp4_scales(torch.from_numpy(s).to(DEV), n, k))
            gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
            bias = (torch.randn(n, device=DEV) * 0.5).to(dtype) if i == 1 else None
            members.append((b, sp, gsd, n) + ((bias,) if bias is not None else ()))
            ref = oracle_ref(kind, a_bits, is_bf16, q, s, gs)
            if bias is not None:
                ref = ref + bias.float().cpu().numpy()[None, :]
            refs.append((ref, oracle_sum_abs(kind, a_bits, is_bf16, q, s, gs)))
        outs = pk.mul_fp4_a16_grouped(name, a, members, m, k, -1)
        for c, (ref, sum_abs) in zip(outs, refs):
            check_gemm(bits(c), ref, is_bf16, sum_abs)
        if k != 2048:
            continue
        h = pk.PetitSolutionHints()
        h.a_type = h.c_type = dtype
        h.b_type = pk.DataType.float4_e2m1 if kind == "nv" else pk.DataType.mxfloat4_e2m1
        mul = pk.mul_nvfp4_a16 if kind == "nv" else pk.mul_mxfp4_a16
        grouped_ids = 0
        for sid in pk.ops.get_fp4_solutions(h, m, ns[0], k):
            try:
                outs = pk.mul_fp4_a16_grouped(name, a, members, m, k, sid)
            except RuntimeError:
                continue            # a kernel kind without a grouped form
            grouped_ids += 1
            for c, mem in zip(outs, members):
                sep = mul(a, mem[0], mem[1], mem[2], m, mem[3], k, sid, bias=mem[4] if len(mem) > 4 else None)
                assert torch.equal(c.view(torch.int16), sep.view(torch.int16)), hex(sid)
        assert grouped_ids >= 3
    with pytest.raises(RuntimeError):
        pk.mul_fp4_a16_grouped(name, a, members * 3, m, k, -1)                      # 9 members
    big = torch.zeros((17, k), dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError):
        pk.mul_fp4_a16_grouped(name, big, members, 17, k, -1)                       # not the decode regime


def test_stacked_mlp_accuracy_budget(pk):
    """The same budget through a STACK: four pre-norm residual MLP layers x <- x + down(silu_mul(gate_up(rmsnorm(x)))), hidden 1024,
    intermediate 2048, 64 tokens, outlier channels in the residual stream (four columns x 40), fresh MXFP4 weights per layer.  The norm and the
    residual run in torch fp32 (not this library's business); the three GEMM paths are the exact default, the native MXFP8 pipeline and the
    native MXFP4 pipeline.  Reported: rms error of the final residual stream against the f64 oracle of the whole stack, relative to its rms --
    how the per-GEMM activation-quantisation error accumulates over depth when a residual path carries the signal."""
    import json
    hid, inter, m, layers = 1024, 2048, 64, 4
    rng = np.random.default_rng(77)
    x0 = rng.standard_normal((m, hid)).astype(np.float32)
    x0[:, rng.choice(hid, 4, replace=False)] *= 40.0
    ws = []
    for layer in range(layers):
        _, q1, s1, _ = random_problem("mx", 1, 2 * inter, hid, 500 + layer, True, mx_band=(123, 127))
        _, q2, s2, _ = random_problem("mx", 1, hid, inter, 600 + layer, True, mx_band=(123, 127))
        ws.append((q1, s1, q2, s2))
    gs1, gs2 = 0.05, 0.02

    def rmsnorm(x):
        return x / np.sqrt((x * x).mean(axis=1, keepdims=True) + 1e-6)

    ref = x0.astype(np.float64)
    for q1, s1, q2, s2 in ws:
        y = rmsnorm(ref) @ O.dequant_mxfp4(q1, s1).astype(np.float64).T * gs1
        h = y[:, :inter] / (1.0 + np.exp(-y[:, :inter])) * y[:, inter:]
        ref = ref + h @ O.dequant_mxfp4(q2, s2).astype(np.float64).T * gs2
    g1, g2 = torch.tensor([gs1], device=DEV), torch.tensor([gs2], device=DEV)
    packed = []
    for q1, s1, q2, s2 in ws:
        packed.append((pk.repack_mxfp4(torch.from_numpy(q1).to(DEV).view(torch.int32), 2 * inter, hid), pk.process_mxfp4_scales(torch.from_numpy(s1).to(DEV), 2 * inter, hid),
                       pk.repack_mxfp4(torch.from_numpy(q2).to(DEV).view(torch.int32), hid, inter), pk.process_mxfp4_scales(torch.from_numpy(s2).to(DEV), hid, inter)))
    report = {}
    for name in ("exact", "mxfp8", "mxfp6", "mxfp4"):
        x = torch.from_numpy(x0).to(DEV)                                  # residual stream in fp32
        for b1, sp1, b2, sp2 in packed:
            xn = (x / torch.sqrt((x * x).mean(dim=1, keepdim=True) + 1e-6)).bfloat16()
            if name == "exact":
                h = pk.mul_mxfp4_a16(xn, b1, sp1, g1, m, 2 * inter, hid, -1, activation="silu_mul")
                d = pk.mul_mxfp4_a16(h, b2, sp2, g2, m, hid, inter, -1)
            else:
                sid = NATIVE_SENTINEL(pk, name)
                hq = pk.mul_mxfp4_native(pk.quantize_activations(xn, name), b1, sp1, g1, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=name)
                d = pk.mul_mxfp4_native(hq, b2, sp2, g2, m, hid, inter, sid)
            x = x + d.float()
        e = x.cpu().numpy().astype(np.float64) - ref
        # the update the four layers added (the residual stream itself is dominated by x0, which every path carries exactly)
        upd = ref - x0
        report[name] = {"rms_err_over_rms_of_stream": float(np.sqrt(np.mean(e ** 2)) / np.sqrt(np.mean(ref ** 2))),
                        "rms_err_over_rms_of_update": float(np.sqrt(np.mean(e ** 2)) / np.sqrt(np.mean(upd ** 2)))}
    print("stacked mlp accuracy budget:", json.dumps(report))
    dump = ROOT / "gpurun_out"
    if dump.is_dir():
        (dump / "stacked_mlp_accuracy_budget.json").write_text(json.dumps({"layers": layers, "hidden": hid, "intermediate": inter, "m": m,
                                                                           "outlier_columns": 4, "outlier_factor": 40, "errors": report}, indent=1))
    assert report["exact"]["rms_err_over_rms_of_update"] <= 2e-2
    assert report["mxfp8"]["rms_err_over_rms_of_update"] <= 0.15
    assert report["mxfp6"]["rms_err_over_rms_of_update"] <= 0.15
    assert report["mxfp4"]["rms_err_over_rms_of_update"] <= 0.8


def _checkpoint_like_layer(pk, fmt, n, k, seed):
    """tools/quantize_weights.py: bf16 weights ~ N(0, 1/K) with heavy-tailed rows and outliers -> NVFP4 / MXFP4 by the checkpoint recipe; returns the
    original weights (f64), the dequantised ones (f64, incl. the global scale), the packed device tensors and the global scale."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import quantize_weights as QW
    w = QW.synthetic_weights(n, k, seed)
    q, sb, gs = (QW.quantize_nvfp4 if fmt == "nvfp4" else QW.quantize_mxfp4)(w)
    qd = torch.from_numpy(q).to(DEV).view(torch.int32)
    if fmt == "nvfp4":
        b, sp = pk.repack_nvfp4(qd, n, k), pk.process_nvfp4_scales(torch.from_numpy(sb).to(DEV).view(torch.float8_e4m3fn), n, k)
        assert np.array_equal(QW.dequantize(fmt, q, sb, 1.0), O.dequant_nvfp4(q, sb).astype(np.float64))      # the tool's dequant IS the oracle's
    else:
        b, sp = pk.repack_mxfp4(qd, n, k), pk.process_mxfp4_scales(torch.from_numpy(sb).to(DEV), n, k)
        assert np.array_equal(QW.dequantize(fmt, q, sb, 1.0), O.dequant_mxfp4(q, sb).astype(np.float64))
    return w.astype(np.float64), QW.dequantize(fmt, q, sb, gs), b, sp, torch.tensor([gs], dtype=torch.float32, device=DEV), QW.stats(fmt, w, q, sb, gs)


def _rel_rms(a, b, denom):
    return float(np.sqrt(np.mean((a - b) ** 2)) / denom)


def test_mlp_block_accuracy_budget_checkpoint_like_weights(pk):
    """VERDICT r04 item 5 / the reference's model-level claim (README.md:3: MMLU 82.15 -> 80.79): the MLP-block budget on weights that look like a
    checkpoint -- bf16 weights N(0, 1/K) with heavy-tailed rows, quantised by tools/quantize_weights.py (the nvidia/*-FP4 recipe for NVFP4, OCP MX
    for MXFP4) -- instead of uniformly random nibbles.  Two errors are kept apart, both relative to the rms of the bf16-weight block's output:
      weight quantisation      the exact FP4 GEMM path against the bf16-WEIGHT block (what the reference's 82.15 -> 80.79 measures), per weight format;
      activation quantisation  the native classes against the exact FP4 path on the same MXFP4 weights (what opting into -2 / -4 / -3 adds)."""
    import json
    hid, inter, m = 2048, 4096, 96
    rng = np.random.default_rng(2027)
    x = rng.standard_normal((m, hid), dtype=np.float32)
    x[:, rng.choice(hid, 6, replace=False)] *= 60.0
    x_bits = O.f32_to_bf16_bits(x)
    xf = to_f32(x_bits, True).astype(np.float64)
    xd = from_bits(x_bits, torch.bfloat16).to(DEV)

    def block(w1, w2, g=1.0):
        y1 = xf @ w1.T
        return (y1[:, :inter] / (1.0 + np.exp(-y1[:, :inter])) * y1[:, inter:]) @ w2.T

    report, wstats = {}, {}
    ref_bf16 = None
    for fmt in ("nvfp4", "mxfp4"):
        w1, dq1, b1, sp1, g1, st1 = _checkpoint_like_layer(pk, fmt, 2 * inter, hid, 31)
        w2, dq2, b2, sp2, g2, st2 = _checkpoint_like_layer(pk, fmt, hid, inter, 32)
        wstats[fmt] = {"gate_up": st1, "down": st2}
        if ref_bf16 is None:
            ref_bf16 = block(w1, w2)
        rms = np.sqrt(np.mean(ref_bf16 ** 2))
        ref_fp4 = block(dq1, dq2)
        mul = pk.mul_nvfp4_a16 if fmt == "nvfp4" else pk.mul_mxfp4_a16
        h1 = mul(xd, b1, sp1, g1, m, 2 * inter, hid, -1, activation="silu_mul")
        y = mul(h1, b2, sp2, g2, m, hid, inter, -1).float().cpu().numpy().astype(np.float64)
        report[f"exact_{fmt}"] = {"weight_quantisation_oracle": _rel_rms(ref_fp4, ref_bf16, rms), "gpu_vs_fp4_oracle": _rel_rms(y, ref_fp4, rms),
                                  "gpu_vs_bf16_weight_block": _rel_rms(y, ref_bf16, rms)}
        if fmt == "mxfp4":
            for act, sid in (("mxfp8", pk.SOLUTION_AUTO_NATIVE_MXFP8), ("mxfp6", pk.SOLUTION_AUTO_NATIVE_MXFP6), ("mxfp4", pk.SOLUTION_AUTO_NATIVE_MXFP4)):
                hq = pk.mul_mxfp4_native(pk.quantize_activations(xd, act), b1, sp1, g1, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=act)
                yn = pk.mul_mxfp4_native(hq, b2, sp2, g2, m, hid, inter, sid).float().cpu().numpy().astype(np.float64)
                report[f"native_{act}"] = {"activation_quantisation_vs_exact_fp4": _rel_rms(yn, ref_fp4, rms), "total_vs_bf16_weight_block": _rel_rms(yn, ref_bf16, rms)}
        else:
            # NVFP4 weights on the native class (round 6): the MFMA-native image re-rounds the weights to e2m3 + one E8M0 per 32 k.  Kept apart: what the
            # re-rounding alone costs (the bf16-activation model on the image's weights against the same model on the true NVFP4 weights), and the class
            # as it runs (image + quantised activations, gate_up emitting the quantised h) against the exact NVFP4 path and the bf16-weight block.
            img1, img2 = pk.nvfp4_native_image(b1, sp1, 2 * inter, hid), pk.nvfp4_native_image(b2, sp2, hid, inter)
            dq1i = pk.offline.nvfp4_native_image_dequant_cpu(img1.cpu(), 2 * inter, hid).numpy().astype(np.float64) * float(g1)
            dq2i = pk.offline.nvfp4_native_image_dequant_cpu(img2.cpu(), hid, inter).numpy().astype(np.float64) * float(g2)
            ref_img = block(dq1i, dq2i)
            report["nvfp4_image"] = {"weight_rerounding_vs_exact_fp4": _rel_rms(ref_img, ref_fp4, rms), "total_vs_bf16_weight_block": _rel_rms(ref_img, ref_bf16, rms),
                                     "weights_moved": float(np.mean(np.abs(dq1i - dq1) > 1e-6 * np.abs(dq1))), "weight_rms_change_over_weight_rms": float(np.sqrt(np.mean((dq1i - dq1) ** 2) / np.mean(dq1 ** 2)))}
            for act, sid in (("mxfp8", pk.SOLUTION_AUTO_NATIVE_MXFP8), ("mxfp6", pk.SOLUTION_AUTO_NATIVE_MXFP6), ("mxfp4", pk.SOLUTION_AUTO_NATIVE_MXFP4)):
                hq = pk.mul_nvfp4_native(pk.quantize_activations(xd, act), img1, g1, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=act)
                yn = pk.mul_nvfp4_native(hq, img2, g2, m, hid, inter, sid).float().cpu().numpy().astype(np.float64)
                report[f"native_nvfp4_{act}"] = {"vs_exact_fp4": _rel_rms(yn, ref_fp4, rms), "vs_image_with_bf16_activations": _rel_rms(yn, ref_img, rms),
                                                 "total_vs_bf16_weight_block": _rel_rms(yn, ref_bf16, rms)}
    print("mlp block accuracy budget (checkpoint-like weights):", json.dumps(report))
    dump = ROOT / "gpurun_out"
    if dump.is_dir():
        (dump / "mlp_accuracy_budget_checkpoint_like.json").write_text(json.dumps({"hidden": hid, "intermediate": inter, "m": m, "outlier_columns": 6, "outlier_factor": 60,
                                                                                    "weights": wstats, "errors_relative_to_rms_of_bf16_weight_block": report}, indent=1))
    for fmt in ("nvfp4", "mxfp4"):
        assert report[f"exact_{fmt}"]["gpu_vs_fp4_oracle"] <= 1e-2                     # the exact path IS the FP4 model
        assert 0.02 <= report[f"exact_{fmt}"]["weight_quantisation_oracle"] <= 0.35     # (a 4-bit weight format costs something: ~10 % per weight)
    assert report["native_mxfp8"]["activation_quantisation_vs_exact_fp4"] <= 8e-2
    assert report["native_mxfp6"]["activation_quantisation_vs_exact_fp4"] <= 0.11
    assert report["native_mxfp4"]["activation_quantisation_vs_exact_fp4"] <= 0.45
    # the deployable classes add less than the weight format already costs
    assert report["native_mxfp8"]["activation_quantisation_vs_exact_fp4"] < report["exact_mxfp4"]["weight_quantisation_oracle"]
    # NVFP4 on its image: the re-rounding alone is a small fraction of what the 4-bit format costs; the class as a whole stays in the MXFP4 class's budgets
    assert report["nvfp4_image"]["weight_rerounding_vs_exact_fp4"] <= 0.3 * report["exact_nvfp4"]["weight_quantisation_oracle"]
    assert report["native_nvfp4_mxfp8"]["vs_exact_fp4"] <= 9e-2 and report["native_nvfp4_mxfp6"]["vs_exact_fp4"] <= 0.12 and report["native_nvfp4_mxfp4"]["vs_exact_fp4"] <= 0.45
    assert report["native_nvfp4_mxfp8"]["total_vs_bf16_weight_block"] <= 1.1 * report["exact_nvfp4"]["gpu_vs_bf16_weight_block"] + 0.02


@pytest.mark.parametrize("wfmt", ["mxfp4", "nvfp4"])
def test_stacked_mlp_accuracy_budget_checkpoint_like_weights(pk, wfmt):
    """(wfmt = nvfp4, round 6: the native classes run on the MFMA-native image of the NVFP4 weights.)  The stacked budget (four pre-norm residual MLP layers, hidden 1024, intermediate 2048, 64 tokens, outlier channels) on checkpoint-like MXFP4
    weights: per path the rms error of the update the four layers add to the residual stream -- against the bf16-WEIGHT stack (weight + activation
    quantisation) and against the exact-FP4 stack (activation quantisation alone)."""
    import json
    hid, inter, m, layers = 1024, 2048, 64, 4
    rng = np.random.default_rng(78)
    x0 = rng.standard_normal((m, hid)).astype(np.float32)
    x0[:, rng.choice(hid, 4, replace=False)] *= 40.0
    L = [(_checkpoint_like_layer(pk, wfmt, 2 * inter, hid, 700 + i), _checkpoint_like_layer(pk, wfmt, hid, inter, 800 + i)) for i in range(layers)]
    nv = wfmt == "nvfp4"
    images = [(pk.nvfp4_native_image(l1[2], l1[3], 2 * inter, hid), pk.nvfp4_native_image(l2[2], l2[3], hid, inter)) for l1, l2 in L] if nv else None
    gain = 8.0       # (N(0, 1/K) weights behind an rmsnorm would add a negligible update: scale the MLP output so that the layers matter)

    def rmsnorm(x):
        return x / np.sqrt((x * x).mean(axis=1, keepdims=True) + 1e-6)

    def stack(which):
        r = x0.astype(np.float64)
        for l1, l2 in L:
            y = rmsnorm(r) @ l1[which].T * gain
            r = r + (y[:, :inter] / (1.0 + np.exp(-y[:, :inter])) * y[:, inter:]) @ l2[which].T * gain
        return r
    ref_bf16, ref_fp4 = stack(0), stack(1)
    upd = np.sqrt(np.mean((ref_bf16 - x0) ** 2))
    report = {"weight_quantisation_oracle": _rel_rms(ref_fp4, ref_bf16, upd)}
    for name in ("exact", "mxfp8", "mxfp6", "mxfp4"):
        x = torch.from_numpy(x0).to(DEV)
        for li, ((_, _, b1, sp1, g1, _), (_, _, b2, sp2, g2, _)) in enumerate(L):
            xn = (x / torch.sqrt((x * x).mean(dim=1, keepdim=True) + 1e-6)).bfloat16()
            ga, gb = g1 * gain, g2 * gain
            if name == "exact":
                mul = pk.mul_nvfp4_a16 if nv else pk.mul_mxfp4_a16
                h = mul(xn, b1, sp1, ga, m, 2 * inter, hid, -1, activation="silu_mul")
                d = mul(h, b2, sp2, gb, m, hid, inter, -1)
            elif nv:
                sid = NATIVE_SENTINEL(pk, name)
                hq = pk.mul_nvfp4_native(pk.quantize_activations(xn, name), images[li][0], ga, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=name)
                d = pk.mul_nvfp4_native(hq, images[li][1], gb, m, hid, inter, sid)
            else:
                sid = NATIVE_SENTINEL(pk, name)
                hq = pk.mul_mxfp4_native(pk.quantize_activations(xn, name), b1, sp1, ga, m, 2 * inter, hid, sid, activation="silu_mul", out_quantized=name)
                d = pk.mul_mxfp4_native(hq, b2, sp2, gb, m, hid, inter, sid)
            x = x + d.float()
        xe = x.cpu().numpy().astype(np.float64)
        report[name] = {"vs_exact_fp4_stack_over_update": _rel_rms(xe, ref_fp4, upd), "vs_bf16_weight_stack_over_update": _rel_rms(xe, ref_bf16, upd)}
    print(f"stacked mlp accuracy budget (checkpoint-like {wfmt} weights):", json.dumps(report))
    dump = ROOT / "gpurun_out"
    if dump.is_dir():
        (dump / ("stacked_mlp_accuracy_budget_checkpoint_like" + ("_nvfp4" if nv else "") + ".json")).write_text(json.dumps({"weights": wfmt, "layers": layers, "hidden": hid, "intermediate": inter, "m": m, "outlier_columns": 4,
                                                                                           "outlier_factor": 40, "mlp_gain": gain, "errors": report}, indent=1))
    assert report["exact"]["vs_exact_fp4_stack_over_update"] <= 2e-2
    # (NVFP4: the image's weight re-rounding rides on top of the activation format -- measured 0.126 / 0.154 / 0.457 against 0.090 / 0.128 / 0.459 for MXFP4 weights)
    assert report["mxfp8"]["vs_exact_fp4_stack_over_update"] <= (0.16 if nv else 0.15)
    assert report["mxfp6"]["vs_exact_fp4_stack_over_update"] <= (0.19 if nv else 0.15)
    assert report["mxfp4"]["vs_exact_fp4_stack_over_update"] <= 0.8
    assert 0.02 <= report["weight_quantisation_oracle"] <= 0.6
    # ... and stays a small part of what the 4-bit weight format itself costs: the total moves by < 10 % of it for the deployable classes
    assert report["mxfp8"]["vs_bf16_weight_stack_over_update"] <= 1.10 * report["exact"]["vs_bf16_weight_stack_over_update"]


def test_examples_run(pk):
    """examples/fp4_linear.py, examples/mxfp4_mlp_pipeline.py and examples/nvfp4_native_prefill.py run to completion on the GPU (their own assertions included)."""
    import subprocess
    import sys
    for name in ("fp4_linear.py", "mxfp4_mlp_pipeline.py", "nvfp4_native_prefill.py"):
        out = subprocess.run([sys.executable, str(ROOT / "examples" / name)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "MISMATCH" not in out.stdout

"""CPU tests of the host side: the packed-layout model, the C ABI surface and the Python
operator layer's argument checking.  No compute call is made (there is no GPU here)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import cdna4_layout as LY
from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n,k", [(16, 256), (48, 512), (64, 1024), (32, 2048), (16, 768)])
def test_layout_model_is_a_bijection_and_matches_index_functions(n, k):
    rng = np.random.default_rng(n * 7 + k)
    qw = rng.integers(0, 2 ** 32, (n, k // 8), dtype=np.uint64).astype(np.uint32)
    pw = LY.pack_weights(qw)
    assert np.array_equal(LY.unpack_weights(pw, n, k), qw)
    for _ in range(300):
        r, c = int(rng.integers(n)), int(rng.integers(k // 8))
        assert pw[LY.weight_word_index(k, r, c)] == qw[r, c]
    s = rng.integers(0, 256, (n, k // 16), dtype=np.uint8)
    ps = LY.pack_nvscales(s, k)
    assert np.array_equal(LY.unpack_nvscales(ps, n, k), s)
    for _ in range(300):
        r, c = int(rng.integers(n)), int(rng.integers(k // 16))
        assert ps[LY.nvscale_byte_index(k, r, c)] == s[r, c]
    m = rng.integers(0, 256, (n, k // 32), dtype=np.uint8)
    pm = LY.pack_mxscales(m, k)
    assert np.array_equal(LY.unpack_mxscales(pm, n, k), m)
    for _ in range(300):
        r, c = int(rng.integers(n)), int(rng.integers(k // 32))
        assert pm[LY.mxscale_byte_index(k, r, c)] == m[r, c]


def test_layout_keeps_the_reference_repack_invariant():
    """dequant(unpack(pack(x))) == dequant(x): the reference's own acceptance test for a packed
    format (quantization_utils_fp4_test.cc:103-133), applied to the gfx950 layout."""
    n, k = 64, 1024
    rng = np.random.default_rng(42)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    s = rng.integers(1, 0x7F, (n, k // 16), dtype=np.uint8)
    qw = q.view(np.uint32).reshape(n, k // 8)
    q2 = LY.unpack_weights(LY.pack_weights(qw), n, k).view(np.uint8).reshape(n, k // 2)
    s2 = LY.unpack_nvscales(LY.pack_nvscales(s, k), n, k)
    assert np.array_equal(O.dequant_nvfp4(q2, s2).view(np.uint32), O.dequant_nvfp4(q, s).view(np.uint32))


def test_span_tiles_rule_matches_layout_h():
    text = (ROOT / "petit-kernel_amd/csrc/layout.h").read_text()
    assert "(k % 1024u == 0) ? 8 : (k % 512u == 0) ? 4 : 2" in text
    assert [LY.span_tiles_for_k(k) for k in (256, 512, 768, 1024, 4096, 28672, 1536)] == [2, 4, 2, 8, 8, 8, 4]


# --- C ABI -------------------------------------------------------------------------

def declared_symbols():
    text = (ROOT / "include/petit_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(petit_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from petit_kernel import _lib
    lib = C.CDLL(str(_lib.LIB_PATH))
    syms = declared_symbols()
    assert len(syms) >= 13
    for name in syms:
        assert hasattr(lib, name), f"{name} declared in include/petit_amd.h but not exported"
    assert set(_lib.EXPORTED_SYMBOLS) == set(syms)


def test_cxx_header_compiles_against_the_c_abi(tmp_path):
    """include/causalflow/petit/gemm.h (the reference's namespace API as inline wrappers)."""
    import subprocess
    src = tmp_path / "t.cc"
    src.write_text('#include "causalflow/petit/gemm.h"\n'
                   "using namespace causalflow::petit::rocm::quantization;\n"
                   "int main() { PetitSolutionHints h{kDataTypeBf16, kDataTypeFp4e2m1, kDataTypeBf16, false};\n"
                   "  unsigned n = 0; SolutionId ids[256];\n"
                   "  if (fp4::GemmGetSolutions(h, 1, 8192, 8192, nullptr, &n) != 0) return 1;\n"
                   "  if (n == 0 || n > 256) return 2; if (fp4::GemmGetSolutions(h, 1, 8192, 8192, ids, &n)) return 3;\n"
                   "  static_assert(sizeof(SolutionId) == 8, \"\");\n"
                   # the reference's helpers (gemm.h:68-104), re-published: Default() = 16 x 64 x 8, fp16 x NVFP4, warps 1 x 2 x 2; MultiStage stores tile_k / 4
                   "  if (SolutionId::Default().Repr() != (1ul | 4ul << 8 | 2ul << 16 | 1ul << 24 | 1ul << 28 | 1ul << 36 | 2ul << 40 | 2ul << 44)) return 5;\n"
                   "  constexpr SolutionId ms = SolutionId::MultiStage(kMatmulFeatures_Grid, kMatmulTypeBMxFp4, kMatmulMfmaTypeBf16, 16, 16, 64, kMatmulWarpPartition_NK, 2, 2, 1);\n"
                   "  if (ms.tile_k != 16 || ms.element_b != kMatmulTypeBMxFp4 || ms.warp_partition_m != 2 || ms.split_k != 0) return 6;\n"
                   "  return ids[0].element_b == kMatmulTypeBNvFp4 && ids[0].mfma_type == kMatmulMfmaTypeBf16 ? 0 : 4; }\n")
    from petit_kernel import _lib
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-I", str(ROOT / "include"), "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", str(src), "-o", str(exe), str(_lib.LIB_PATH),
                    f"-Wl,-rpath,{_lib.LIB_PATH.parent}", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_solution_enumeration_and_ids():
    from petit_kernel import _lib
    import petit_kernel
    sols = petit_kernel.get_fp4_solutions(1, 8192, 8192, torch.bfloat16, torch.bfloat16)
    assert len(sols) == len(set(sols)) > 4
    for s in sols:
        assert (s >> 28) & 0xF == 1 and (s >> 32) & 0xF == 1  # element_b NvFp4, mfma bf16 (gemm.h:14-24)
        assert (s >> 24) & 0xF == 3                           # Grid | HighPrecision (gemm.h:8-12)
        assert "bf16xnvfp4" in _lib.describe_solution(s)  # "stream ..." or "tiled ..."
    # both call shapes of the reference
    h = petit_kernel.PetitSolutionHints()
    h.a_type = petit_kernel.DataType.float16
    h.b_type = petit_kernel.DataType.float4_e2m1
    h.c_type = petit_kernel.DataType.float16
    via_hints = petit_kernel.ops.get_fp4_solutions(h, 4, 4096, 4096)
    assert via_hints == petit_kernel.get_fp4_solutions(4, 4096, 4096, torch.float16, torch.float16)
    assert all((s >> 32) & 0xF == 0 for s in via_hints)
    # K % 1024 != 0 selects the other span sizes; K % 256 != 0 has no solution
    assert petit_kernel.get_fp4_solutions(1, 64, 768, torch.bfloat16, torch.bfloat16)
    assert petit_kernel.get_fp4_solutions(1, 64, 384, torch.bfloat16, torch.bfloat16) == []
    # non-FP4 b_type: -1 like algo_chooser.cc:20-23
    bad = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, 0, _lib.CXX_DTYPE_BF16, 0)
    cnt = C.c_uint(0)
    assert _lib.lib.petit_gemm_get_solutions(C.byref(bad), 1, 64, 256, None, C.byref(cnt)) == -1
    auto = _lib.lib.petit_gemm_default_solution(C.byref(_lib.SolutionHints(5, 3, 5, 0)), 1, 8192, 8192)
    assert auto in sols


def test_mxfp4_f16range_dtype_is_an_alias_without_a_gpu():
    """PETIT_DTYPE_MXFP4_E2M1_F16RANGE (round 3: a caller's promise that selected a kernel family) is a deprecated alias of plain MXFP4: the fp16
    kernels test the scale range themselves.  Header value = Python value; same ids, same default, the full kernel set for fp16 activations."""
    import re
    from petit_kernel import _lib
    hdr = (ROOT / "include" / "petit_amd.h").read_text()
    assert int(re.search(r"PETIT_DTYPE_MXFP4_E2M1_F16RANGE = (\d+)", hdr).group(1)) == _lib.CXX_DTYPE_MXFP4_E2M1_F16RANGE == 8
    assert (int(re.search(r"PETIT_MXFP4_F16RANGE_SCALE_MIN (\d+)", hdr).group(1)), int(re.search(r"PETIT_MXFP4_F16RANGE_SCALE_MAX (\d+)", hdr).group(1))) == \
        (_lib.MXFP4_F16RANGE_SCALE_MIN, _lib.MXFP4_F16RANGE_SCALE_MAX) == (114, 140)
    # 0.5 * 2^(114 - 127) is the smallest normal fp16, 6 * 2^(140 - 127) the largest product below 65504
    assert np.float16(0.5 * 2.0 ** (114 - 127)) == np.float16(2.0 ** -14) and 6 * 2.0 ** (140 - 127) < 65504 < 6 * 2.0 ** (141 - 127)

    def ids(a, b, m=16, n=8192, k=8192):
        h = _lib.SolutionHints(a, b, a, 0)
        cnt = C.c_uint(0)
        assert _lib.lib.petit_gemm_get_solutions(C.byref(h), m, n, k, None, C.byref(cnt)) == 0
        buf = (C.c_uint64 * max(cnt.value, 1))()
        assert _lib.lib.petit_gemm_get_solutions(C.byref(h), m, n, k, buf, C.byref(cnt)) == 0
        return [int(buf[i]) for i in range(cnt.value)]
    for a in (_lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_BF16):
        plain, alias = ids(a, _lib.CXX_DTYPE_MXFP4_E2M1), ids(a, _lib.CXX_DTYPE_MXFP4_E2M1_F16RANGE)
        assert plain and plain == alias and all((i >> 28) & 0xF == 2 for i in plain)
    f16 = ids(_lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_MXFP4_E2M1)
    assert any((i >> 36) & 0xF == 2 and (i >> 48) & 0xF in (10, 11) for i in f16)   # the shared-tile kernel
    assert any((i >> 48) & 0xF == 12 for i in ids(_lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_MXFP4_E2M1, m=512))   # the 32x32x16 kernels
    dflt = [_lib.lib.petit_gemm_default_solution(C.byref(_lib.SolutionHints(4, b, 4, 0)), 16, 8192, 8192) for b in (7, 8)]
    assert dflt[0] == dflt[1] and (dflt[0] & ~(0xF << 60)) | (1 << 60) in f16
    # an id written with round 3's element nibble (3) still names its kernel
    old = (f16[0] & ~(0xF << 28)) | (3 << 28)
    assert _lib.describe_solution(old) == _lib.describe_solution(f16[0])


def test_error_codes_without_a_gpu():
    """Paths that return before any launch: zero sizes, bad shapes, unknown ids."""
    from petit_kernel import _lib
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    f = _lib.lib.petit_gemm_fp4_fp16_grid
    one = C.c_void_p(16)  # never dereferenced on these paths
    auto = C.c_uint64(_lib.PETIT_SOLUTION_AUTO)
    assert f(one, one, one, one, one, 0, 64, 256, C.byref(h), auto, None) == 0  # gemm_fp4_fp16_grid.cc:42-44
    assert f(one, one, one, one, one, 1, 0, 256, C.byref(h), auto, None) == 0
    assert f(one, one, one, one, one, 1, 40, 256, C.byref(h), auto, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert f(one, one, one, one, one, 1, 64, 100, C.byref(h), auto, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert f(one, one, one, one, one, 1, 64, 256, C.byref(h), C.c_uint64(0x1234), None) == _lib.PETIT_ERROR_KERNEL_SHAPE
    assert f(None, one, one, one, one, 1, 64, 256, C.byref(h), auto, None) == _lib.PETIT_ERROR_BAD_ARGUMENT
    hx = _lib.SolutionHints(_lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    assert f(one, one, one, one, one, 1, 64, 256, C.byref(hx), auto, None) == _lib.PETIT_ERROR_KERNEL_SHAPE
    for fn in (_lib.lib.petit_repack_nvfp4_weights, _lib.lib.petit_repack_nvfp4_scales,
               _lib.lib.petit_repack_mxfp4_scales):
        assert fn(one, one, 0, 64, None) == 0
        assert fn(one, one, 256, 24, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert _lib.lib.petit_repack_nvfp4_scales(one, one, 128, 16, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert _lib.error_string(1) == "incompatible problem shape"
    assert _lib.lib.petit_layout_tag() == b"petit-cdna4/1"


def test_python_layer_argument_checks():
    """Same RuntimeError texts as the pybind layer (lib/pybind/fp4.cc:38-260)."""
    import petit_kernel
    qw = torch.zeros((64, 32), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="size_k = 200 is not divisible by tile_k_size = 128"):
        petit_kernel.repack_nvfp4(qw, 64, 200)
    with pytest.raises(RuntimeError, match="size_n = 60 is not divisible by tile_n_size = 16"):
        petit_kernel.repack_nvfp4(qw, 60, 256)
    with pytest.raises(RuntimeError, match="b_q_weight is not on GPU"):
        petit_kernel.repack_nvfp4(qw, 64, 256)
    with pytest.raises(RuntimeError, match="Shape mismatch"):
        petit_kernel.repack_nvfp4(qw, 64, 512)
    s = torch.zeros((64, 16), dtype=torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="scales is not on GPU"):
        petit_kernel.process_nvfp4_scales(s, 64, 256)
    with pytest.raises(RuntimeError, match="Only groupsize = 16 is supported"):
        petit_kernel.process_nvfp4_scales(s, 64, 512)
    with pytest.raises(RuntimeError, match="tile_k_size = 256"):
        petit_kernel.process_nvfp4_scales(s, 64, 128)
    mx = torch.zeros((64, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="Only groupsize = 32 is supported"):
        petit_kernel.process_mxfp4_scales(mx, 64, 512)
    with pytest.raises(RuntimeError, match="scales is not on GPU"):
        petit_kernel.process_mxfp4_scales(mx, 64, 256)
    a = torch.zeros((1, 256), dtype=torch.float32)
    with pytest.raises(RuntimeError, match="A must be bfloat16 or float16"):
        petit_kernel.mul_nvfp4_a16(a, qw, s, torch.ones(1), 1, 64, 256, -1)
    with pytest.raises(RuntimeError, match="Only groupsize = 16 is supported"):
        petit_kernel.mul_nvfp4_a16(a.bfloat16(), qw, s, torch.ones(1), 1, 64, 512, -1)
    assert [d.value for d in petit_kernel.DataType] == [0, 1, 2, 3, 4, 5, 6]  # __init__.py:8-15


# --- offline (host-memory) repack: SURVEY.md section 8f-4 ---------------------------------------

@pytest.mark.parametrize("n,k", [(16, 256), (64, 256), (128, 512), (96, 768), (256, 1024), (32, 2048)])
def test_offline_repack_matches_the_layout_model(n, k):
    """The C-ABI host twins of the repack entry points produce exactly the packed layout (no GPU)."""
    import petit_kernel
    rng = np.random.default_rng(n * 7 + k)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    s = rng.integers(0, 256, (n, k // 16), dtype=np.uint8)
    mx = rng.integers(0, 256, (n, k // 32), dtype=np.uint8)
    b = petit_kernel.offline.repack_nvfp4_cpu(torch.from_numpy(q).view(torch.int32), n, k)
    assert b.shape == (n // 16, 2 * k) and b.dtype == torch.int32 and not b.is_cuda
    assert np.array_equal(b.numpy().view(np.uint32).ravel(), LY.pack_weights(q.view(np.uint32).reshape(n, k // 8)))
    sp = petit_kernel.offline.process_nvfp4_scales_cpu(torch.from_numpy(s).view(torch.float8_e4m3fn), n, k)
    assert sp.shape == (n, k // 16) and sp.dtype == torch.float8_e4m3fn
    assert np.array_equal(sp.view(torch.uint8).numpy().ravel(), LY.pack_nvscales(s, k))
    if n % 32 == 0:
        mp = petit_kernel.offline.process_mxfp4_scales_cpu(torch.from_numpy(mx), n, k)
        assert mp.shape == (n // 32, k) and mp.dtype == torch.uint8
        assert np.array_equal(mp.numpy().ravel(), LY.pack_mxscales(mx, k))


def test_offline_repack_argument_checks():
    import petit_kernel
    q = torch.zeros((16, 32), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="size_k = 200 is not divisible"):
        petit_kernel.offline.repack_nvfp4_cpu(q, 16, 200)
    with pytest.raises(RuntimeError, match="qw must be"):
        petit_kernel.offline.repack_nvfp4_cpu(q, 32, 256)
    with pytest.raises(RuntimeError, match="not divisible by 32"):
        petit_kernel.offline.process_mxfp4_scales_cpu(torch.zeros((16, 8), dtype=torch.uint8), 16, 256)
    from petit_kernel import _lib
    buf = (C.c_uint * 16)()
    assert _lib.lib.petit_repack_nvfp4_weights_host(buf, buf, 128, 16) == 4      # in place: bad argument
    assert _lib.lib.petit_repack_nvfp4_weights_host(buf, None, 128, 16) == 4
    assert _lib.lib.petit_repack_nvfp4_scales_host(buf, None, 0, 0) == 0         # empty problem


def test_epilogue_struct_is_validated_without_a_gpu():
    """petit_gemm_*_ex rejects epilogue fields it does not implement before touching the device."""
    from petit_kernel import _lib
    hints = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    for fn in (_lib.lib.petit_gemm_fp4_fp16_grid_ex, _lib.lib.petit_gemm_mxfp4_fp16_grid_ex):
        epi = _lib.Epilogue(None, 7, 0)                       # an activation nobody implements
        assert fn(None, None, None, None, None, 1, 64, 256, C.byref(hints), C.c_uint64(_lib.PETIT_SOLUTION_AUTO),
                  C.byref(epi), None) == _lib.PETIT_ERROR_BAD_ARGUMENT
        epi = _lib.Epilogue(None, 1, 0)                       # SiLU-mul needs gate / up halves of whole n-tiles
        fake = C.c_void_p(256)                                # never dereferenced: the shape check comes first
        assert fn(fake, fake, fake, fake, fake, 1, 48, 256, C.byref(hints), C.c_uint64(_lib.PETIT_SOLUTION_AUTO),
                  C.byref(epi), None) == _lib.PETIT_ERROR_PROBLEM_SHAPE
        epi = _lib.Epilogue(None, 0, 0)                       # empty problem: ok, nothing enqueued
        assert fn(None, None, None, None, None, 0, 64, 256, C.byref(hints), C.c_uint64(_lib.PETIT_SOLUTION_AUTO),
                  C.byref(epi), None) == 0


# --- arch table (csrc/hal.hip): built-in rows and the $PETIT_AMD_TUNE_FILE override ----------------

def _default_solution_in_subprocess(env_extra, a_type, b_type, m, n, k):
    import os
    import subprocess
    import sys
    code = ("import sys, ctypes as C; sys.path.insert(0, r'%s'); from petit_kernel import _lib; "
            "h = _lib.SolutionHints(%d, %d, %d, 0); print('%%x' %% _lib.lib.petit_gemm_default_solution(C.byref(h), %d, %d, %d))"
            % (ROOT / "petit-kernel_amd", a_type, b_type, a_type, m, n, k))
    env = dict(os.environ, **env_extra)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    return int(out.strip().splitlines()[-1], 16)


# The M a table row was measured at (tools/make_tuned_inc.py BUCKET): the upper end of its bucket, 2048 / 8192 for the two prefill buckets whose
# upper end is not a measurement.  At THAT M solution_id = -1 resolves to exactly the row; elsewhere in the bucket to the same kernel, possibly with
# a smaller K split (csrc/api.hip guarded_splitk).
def row_rep_m(lo, hi):
    # ((49, 64): what is left of a 33-64 row after a 48-row kernel took 33-48: still measured at 64)
    return 8192 if hi == 1 << 20 else 2048 if (lo, hi) == (1025, 4096) else hi


def same_kernel_split_at_most(got, row):
    return (got ^ row) & ~(0xF << 60) == 0 and 1 <= (got >> 60) <= (row >> 60)


def test_arch_table_rows_and_tune_file_override(tmp_path):
    """solution_id = -1 consults the measured table first (every row must name a kernel that exists and fits),
    and a $PETIT_AMD_TUNE_FILE row written in tools/tune.py's format takes precedence over it."""
    from petit_kernel import _lib
    rows = re.findall(r"\{(\d+), (\d+), (\d+)u, (\d+)u, (\d+)u, (\d+)u, 0x([0-9a-f]+)ull\}",
                      (ROOT / "petit-kernel_amd/csrc/tuned_gfx950.inc").read_text())
    assert len(rows) >= 100
    prefill_kernels = {}
    for at, bt, n, k, lo, hi, sol in rows:
        if int(hi) > 512:
            prefill_kernels.setdefault((int(at), int(bt), int(n), int(k)), set()).add((int(sol, 16) & ~(0xF << 60)) | (1 << 60))
    for at, bt, n, k, lo, hi, sol in rows:
        at, bt, n, k, lo, hi, sol = int(at), int(bt), int(n), int(k), int(lo), int(hi), int(sol, 16)
        hints = _lib.SolutionHints(at, bt, at, 0)
        assert (sol >> 48) & 0xF not in (9, 13), "a native-FP4 kernel must never be a default"   # (as tools/make_tuned_inc.py)
        assert _lib.lib.petit_gemm_default_solution(C.byref(hints), row_rep_m(lo, hi), n, k) == sol, (at, bt, n, k, lo, hi, hex(sol))
        for m in {lo, min(hi, lo + 3)}:
            got = _lib.lib.petit_gemm_default_solution(C.byref(hints), m, n, k)
            if hi <= 512:
                assert same_kernel_split_at_most(got, sol), (at, bt, n, k, m, hex(sol))
            else:   # prefill: at a ragged M a sibling row's kernel may take over when its grid quantises > 8 % better (csrc/api.hip choose_auto)
                assert same_kernel_split_at_most(got, sol) or got in prefill_kernels[(at, bt, n, k)], (at, bt, n, k, m, hex(sol), hex(got))
            assert "unknown" not in _lib.describe_solution(sol)
    # override: pick some other enumerated kernel for one of the table's shapes
    at, bt, n, k, lo, hi, sol = rows[0]
    at, bt, n, k, lo, sol = int(at), int(bt), int(n), int(k), int(lo), int(sol, 16)
    hints = _lib.SolutionHints(at, bt, at, 0)
    cnt = C.c_uint(0)
    assert _lib.lib.petit_gemm_get_solutions(C.byref(hints), lo, n, k, None, C.byref(cnt)) == 0
    ids = (C.c_uint64 * cnt.value)()
    assert _lib.lib.petit_gemm_get_solutions(C.byref(hints), lo, n, k, ids, C.byref(cnt)) == 0
    other = next(i for i in ids if i != sol)
    tune = tmp_path / "tune.txt"
    tune.write_text(f"# a_type b_type n k m_lo m_hi solution\n{at} {bt} {n} {k} {lo} {lo} {other:x}\n")
    assert _default_solution_in_subprocess({"PETIT_AMD_TUNE_FILE": str(tune)}, at, bt, lo, n, k) == other
    assert _default_solution_in_subprocess({"PETIT_AMD_TUNE_FILE": ""}, at, bt, lo, n, k) == sol
    # a file saved by a round 1-4 build: its open-ended "257 .. 2^20" row keeps the bucket it was measured in and no longer hides the prefill buckets
    # this build measures separately
    pre = next(r for r in rows if int(r[4]) == 4097)
    at, bt, n, k, sol = int(pre[0]), int(pre[1]), int(pre[2]), int(pre[3]), int(pre[6], 16)
    hints = _lib.SolutionHints(at, bt, at, 0)
    cnt = C.c_uint(0)
    _lib.lib.petit_gemm_get_solutions(C.byref(hints), 512, n, k, None, C.byref(cnt))
    ids = (C.c_uint64 * cnt.value)()
    _lib.lib.petit_gemm_get_solutions(C.byref(hints), 512, n, k, ids, C.byref(cnt))
    old_pick = next(i for i in ids if (i >> 48) & 0xF == 8 and i != sol)
    tune.write_text(f"{at} {bt} {n} {k} 257 {1 << 20} {old_pick:x}\n")
    assert _default_solution_in_subprocess({"PETIT_AMD_TUNE_FILE": str(tune)}, at, bt, 512, n, k) == old_pick
    assert _default_solution_in_subprocess({"PETIT_AMD_TUNE_FILE": str(tune)}, at, bt, 8192, n, k) == sol


def test_tune_file_native_row_is_ignored_for_auto(tmp_path):
    """PETIT_SOLUTION_AUTO never runs a native-FP4 kernel (different accuracy class), even when a tune file produced
    with `tools/tune.py --native` names one: the row is skipped and the exact-kernel choice stands."""
    from petit_kernel import _lib
    at, bt, m, n, k = _lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, 512, 8192, 8192
    hints = _lib.SolutionHints(at, bt, at, 0)
    want = _lib.lib.petit_gemm_default_solution(C.byref(hints), m, n, k)
    assert want and (want >> 48) & 0xF != 9
    _lib.lib.petit_enable_native_fp4(1)
    try:
        cnt = C.c_uint(0)
        assert _lib.lib.petit_gemm_get_solutions(C.byref(hints), m, n, k, None, C.byref(cnt)) == 0
        ids = (C.c_uint64 * cnt.value)()
        assert _lib.lib.petit_gemm_get_solutions(C.byref(hints), m, n, k, ids, C.byref(cnt)) == 0
    finally:
        _lib.lib.petit_enable_native_fp4(0)
    for kind in (9, 13):   # the 16x16x128 and the 32x32x64 native kernels
        native = next(i for i in ids if (i >> 48) & 0xF == kind)
        tune = tmp_path / f"tune{kind}.txt"
        tune.write_text(f"{at} {bt} {n} {k} {m} {m} {native:x}\n")
        got = _default_solution_in_subprocess({"PETIT_AMD_TUNE_FILE": str(tune), "PETIT_AMD_NATIVE_FP4": "1"}, at, bt, m, n, k)
        assert got == want, (kind, hex(got), hex(want))


def test_workspace_bytes_query():
    """petit_gemm_workspace_bytes: 0 for plain kernels, splitk * m * n * 4 for a cross-workgroup K split (stream and
    tiled kernels), quantised activations (+ slabs) for the native kernels."""
    from petit_kernel import _lib
    at, bt, m, n, k = _lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, 512, 8192, 8192
    hints = _lib.SolutionHints(at, bt, at, 0)
    _lib.lib.petit_enable_native_fp4(1)
    try:
        cnt = C.c_uint(0)
        _lib.lib.petit_gemm_get_solutions(C.byref(hints), m, n, k, None, C.byref(cnt))
        ids = (C.c_uint64 * cnt.value)()
        _lib.lib.petit_gemm_get_solutions(C.byref(hints), m, n, k, ids, C.byref(cnt))
    finally:
        _lib.lib.petit_enable_native_fp4(0)
    need = lambda sid: _lib.lib.petit_gemm_workspace_bytes(C.byref(hints), m, n, k, C.c_uint64(sid))
    with_split = lambda sid, sk: (sid & ~(0xF << 60)) | (sk << 60)
    stream = next(i for i in ids if (i >> 48) & 0xF == 0)
    tiled = next(i for i in ids if (i >> 48) & 0xF == 8)
    native = next(i for i in ids if (i >> 48) & 0xF == 9)
    assert need(stream) == 0 and need(tiled) == 0
    assert need(with_split(stream, 2)) == 2 * m * n * 4 and need(with_split(tiled, 4)) == 4 * m * n * 4
    nat = _lib.lib.petit_native_workspace_bytes(m, k)
    assert need(native) == nat == m * k + m * k // 32
    assert need(with_split(native, 2)) == ((nat + 255) & ~255) + 2 * m * n * 4
    assert need(0x1234) == 0


@pytest.mark.parametrize("n,k", [(64, 256), (128, 512), (192, 1024), (64, 2048)])
def test_ingest_of_reference_packed_tensors(n, k):
    """A checkpoint already repacked by the REFERENCE wheel converts to this build's layout on the host
    (petit_convert_reference_*): the oracle's restatement of the reference's packed formats (PetitFormat nibble
    re-encode + RepackQWeightLayout64x32, the e4m3 -> "e5m3" scale bytes, the MX scale layout) produces the input,
    and the result must equal this build's own repack of the native tensors, byte for byte (modulo the sign of zero,
    which the reference's format drops)."""
    import petit_kernel
    rng = np.random.default_rng(n + k)
    q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
    q_nozero_sign = q.copy()                                   # the reference stores -0 as +0: compare on that form
    lo, hi = q_nozero_sign & 0x0F, q_nozero_sign >> 4
    lo[lo == 8] = 0
    hi[hi == 8] = 0
    q_nozero_sign = (lo | (hi << 4)).astype(np.uint8)
    ref_w = O.petit_repack_weights(q.view(np.uint32).reshape(n, k // 8))
    got_w = petit_kernel.offline.from_reference_packed_weights(torch.from_numpy(ref_w.view(np.int32)).reshape(n // 16, 2 * k), n, k)
    want_w = petit_kernel.offline.repack_nvfp4_cpu(torch.from_numpy(q_nozero_sign).view(torch.int32), n, k)
    assert torch.equal(got_w, want_w)
    s = rng.integers(0, 0x7F, (n, k // 16), dtype=np.uint8)   # every non-negative, non-NaN e4m3 byte (incl. subnormals)
    ref_s = O.petit_repack_nvscales(s, k)
    got_s = petit_kernel.offline.from_reference_packed_nvfp4_scales(torch.from_numpy(ref_s).reshape(n, k // 16), n, k)
    want_s = petit_kernel.offline.process_nvfp4_scales_cpu(torch.from_numpy(s).view(torch.float8_e4m3fn), n, k)
    assert torch.equal(got_s.view(torch.uint8), want_s.view(torch.uint8))
    mx = rng.integers(0, 256, (n, k // 32), dtype=np.uint8)
    ref_mx = O.petit_repack_mxscales(mx, k)
    got_mx = petit_kernel.offline.from_reference_packed_mxfp4_scales(torch.from_numpy(ref_mx).reshape(n // 32, k), n, k)
    assert torch.equal(got_mx, petit_kernel.offline.process_mxfp4_scales_cpu(torch.from_numpy(mx), n, k))


def test_compiled_ops_have_shape_functions_for_tracing():
    """torch.ops.petit_kernel.* carry Meta kernels (csrc/torch_binding.cpp): with meta tensors, and under FakeTensorMode with
    fake GPU tensors (what torch.compile / torch.export trace with), every op returns the shape, dtype and device the real
    kernel would, and launches nothing -- this runs on a box without a GPU.  A CPU tensor still gets the reference's own
    error text (lib/pybind/fp4.cc:50-52), not a dispatcher message."""
    from petit_kernel import compiled
    from torch._subclasses.fake_tensor import FakeTensorMode
    if not compiled.available():
        pytest.skip(f"compiled binding not built: {compiled.why_unavailable()}")
    m, n, k = 5, 256, 1024

    def run(dev):
        a = torch.empty((m, k), dtype=torch.bfloat16, device=dev)
        q = torch.empty((n, k // 8), dtype=torch.int32, device=dev)
        b = torch.ops.petit_kernel.repack_nvfp4(q, n, k)
        assert b.shape == (n // 16, 2 * k) and b.dtype == torch.int32
        s = torch.ops.petit_kernel.process_nvfp4_scales(torch.empty((n, k // 16), dtype=torch.float8_e4m3fn, device=dev), n, k)
        assert s.shape == (n, k // 16) and s.dtype == torch.float8_e4m3fn
        sx = torch.ops.petit_kernel.process_mxfp4_scales(torch.empty((n, k // 32), dtype=torch.uint8, device=dev), n, k)
        assert sx.shape == (n // 32, k) and sx.dtype == torch.uint8
        gs = torch.empty(1, device=dev)
        c = torch.ops.petit_kernel.mul_nvfp4_a16(a, b, s, gs, m, n, k, -1)
        assert c.shape == (m, n) and c.dtype == a.dtype and c.device == a.device
        c = torch.ops.petit_kernel.mul_mxfp4_a16(a.half(), b, sx, gs, m, n, k, -1, None, 1)
        assert c.shape == (m, n // 2) and c.dtype == torch.float16
        return c

    assert run("meta").device.type == "meta"
    with FakeTensorMode():
        assert run("cuda").device.type == "cuda"
    with pytest.raises(RuntimeError, match="not on GPU"):
        torch.ops.petit_kernel.repack_nvfp4(torch.zeros((n, k // 8), dtype=torch.int32), n, k)


def test_unseen_shapes_stay_close_to_the_measured_best():
    """Where the arch table has no row: (1) the kernel of the nearest tabulated shapes (hal.h tuned_nearest_list, ranked in api.hip choose_auto), replayed on the
    ten shapes that tools/build_table.py kept out of the table against every candidate the in-library tuner timed on them on MI355X in a LATER session than the
    ones the table was built in (profiles/r05_heldout_final_candidates.csv.gz, all 13 M buckets incl. prefill; round 4 replayed the table-building session itself,
    which flatters the picks): within 6 % of the best kernel in the median of every M bucket, 12 % at the 90th percentile overall, 25 % at the 90th percentile of
    every bucket, never worse than 1.4 x (the neighbours are ranked by how their kernels' grids fit THIS problem: api.hip grid_overhead); (2) the formula heuristic behind
    it (table disabled), on the round-4 log of all 3680 tabulated problems: median within 4 %, 90 % within 25 %."""
    import subprocess
    import sys

    def run(*args):
        out = subprocess.run([sys.executable, str(ROOT / "tools" / "check_heuristic.py"), *args], capture_output=True, text=True, check=True).stdout
        m = re.search(r"slowdown vs best: median ([0-9.]+), p90 ([0-9.]+), max ([0-9.]+)", out)
        assert m, out
        buckets = [tuple(float(x) for x in b) for b in re.findall(r"^\| \d+-\d* \| \d+ \| ([0-9.]+) \| ([0-9.]+) \| ([0-9.]+) \|$", out, re.M)]
        return tuple(float(x) for x in m.groups()), buckets, out
    (median, p90, worst), buckets, out = run("--heldout", "--by-m", "--mode", "nearest")
    assert len(buckets) == 13 and median <= 1.02 and p90 <= 1.12 and worst <= 1.40 and all(b[0] <= 1.06 for b in buckets), out
    assert all(b[1] <= 1.25 for b in buckets), out                     # the tail: p90 of every bucket (measured 1.06-1.25; 1.05-1.35 with the nearest row taken blindly)
    (median, p90, _), buckets, out = run("--by-m", "--data", str(ROOT / "profiles" / "r04_table_candidates.csv.gz"))
    assert len(buckets) == 10 and median <= 1.04 and p90 <= 1.25 and all(b[0] <= 1.06 for b in buckets), out


def test_builtin_tables_parse_and_name_kernels_of_this_build():
    """csrc/tuned_gfx950.inc (>= 1500 rows: the linear shapes of seven model families at TP 1 / 2 / 4 / 8, tools/build_table.py) and
    csrc/cost_gfx950.inc: every row parses, names a kernel this build has (petit_describe_solution) that fits the row's span size, M
    ranges of one problem do not overlap, and the library serves each row's own problem with exactly that kernel."""
    from petit_kernel import _lib
    text = (ROOT / "petit-kernel_amd" / "csrc" / "tuned_gfx950.inc").read_text()
    rows = re.findall(r"^\{(\d+), (\d+), (\d+)u, (\d+)u, (\d+)u, (\d+)u, 0x([0-9a-f]+)ull\},$", text, re.M)
    assert len(rows) >= 1500 and len(rows) == sum(1 for ln in text.splitlines() if ln.startswith("{"))
    seen = {}
    shapes = set()
    for at, bt, n, k, lo, hi, sid in rows:
        at, bt, n, k, lo, hi, sid = int(at), int(bt), int(n), int(k), int(lo), int(hi), int(sid, 16)
        assert at in (4, 5) and bt in (3, 7) and n % 16 == 0 and k % 256 == 0 and 1 <= lo <= hi
        assert not _lib.describe_solution(sid).startswith("unknown"), hex(sid)
        assert (sid >> 48) & 0xF not in (9, 13)                               # never a native-FP4 kernel in the exact class's table
        assert ((sid >> 16) & 0x1F) // 2 == (8 if k % 1024 == 0 else 4 if k % 512 == 0 else 2)
        for (lo2, hi2) in seen.setdefault((at, bt, n, k), []):
            assert hi < lo2 or lo > hi2, (at, bt, n, k, lo, hi)
        seen[(at, bt, n, k)].append((lo, hi))
        shapes.add((n, k))
    assert len(shapes) >= 80
    for at, bt, n, k, lo, hi, sid in rows[::37]:                              # a sample through the ABI: the row is what AUTO resolves to
        h = _lib.SolutionHints(int(at), int(bt), int(at), 0)
        assert _lib.lib.petit_gemm_default_solution(C.byref(h), row_rep_m(int(lo), int(hi)), int(n), int(k)) == int(sid, 16)
    cost = (ROOT / "petit-kernel_amd" / "csrc" / "cost_gfx950.inc").read_text()
    crow = re.findall(r"^\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), ([0-9.]+)f, ([0-9.]+)f, ([0-9.]+)f\},$", cost, re.M)
    assert len(crow) >= 40 and len(crow) == sum(1 for ln in cost.splitlines() if ln.startswith("{"))
    assert all(0.1 < float(r[8]) < 10 and 1.0 <= float(r[9]) <= 2.0 and float(r[10]) < 0.2 for r in crow)
    # an unseen shape takes its nearest neighbour's kernel (here: Llama-3-70B qkv for a 10368 x 8192 problem), unless that is switched off
    h = _lib.SolutionHints(5, 3, 5, 0)
    assert _lib.lib.petit_gemm_default_solution(C.byref(h), 16, 10368, 8192) == _lib.lib.petit_gemm_default_solution(C.byref(h), 16, 10240, 8192)


# --- tune-and-persist plumbing (csrc/tune.hip, hal.hip): everything that needs no GPU ----------------

def test_run_time_tune_rows_round_trip(tmp_path):
    """petit_tune_insert -> what PETIT_SOLUTION_AUTO resolves to changes at once (the per-thread pick cache is keyed on the
    table's generation); petit_tune_save writes the $PETIT_AMD_TUNE_FILE format; a fresh process that names the file picks the
    same kernel on its first call; the memoised workspace query follows the new pick."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, ctypes as C
sys.path.insert(0, r'%s')
from petit_kernel import _lib
L = _lib.lib
at, bt, m, n, k = _lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, 128, 3072, 5120       # a shape no built-in row names
h = _lib.SolutionHints(at, bt, at, 0)
before = L.petit_gemm_default_solution(C.byref(h), m, n, k)
cnt = C.c_uint(0); L.petit_gemm_get_solutions(C.byref(h), m, n, k, None, C.byref(cnt))
ids = (C.c_uint64 * cnt.value)(); L.petit_gemm_get_solutions(C.byref(h), m, n, k, ids, C.byref(cnt))
tiled = next(i for i in ids if (i >> 48) & 0xF == 8 and i != before)
pick = (tiled & ~(0xF << 60)) | (4 << 60)                                                  # with a K split of 4: needs scratch
g0 = L.petit_tune_generation()
assert L.petit_gemm_workspace_bytes(C.byref(h), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)) == L.petit_gemm_workspace_bytes(C.byref(h), m, n, k, C.c_uint64(before))
assert L.petit_tune_insert(C.byref(h), n, k, 65, 128, C.c_uint64(pick)) == 0
assert L.petit_tune_generation() > g0
assert L.petit_gemm_default_solution(C.byref(h), m, n, k) == pick
assert L.petit_gemm_default_solution(C.byref(h), 64, n, k) != pick                         # outside the row's M range
assert L.petit_gemm_workspace_bytes(C.byref(h), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)) == 4 * m * n * 4
# a caller without scratch gets the best kernel that needs none -- and resolve_solution says which
no_ws = L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None, C.c_uint64(0))
assert no_ws and (no_ws >> 60) == 1 and no_ws != pick
assert L.petit_tune_insert(C.byref(h), n, k, 65, 128, C.c_uint64(0x1234)) == _lib.PETIT_ERROR_KERNEL_SHAPE   # not a kernel id
assert L.petit_tune_insert(C.byref(h), n, k, 0, 128, C.c_uint64(pick)) == _lib.PETIT_ERROR_BAD_ARGUMENT
assert L.petit_tune_save(sys.argv[1].encode()) == 0
print('%%x' %% pick)
""" % (ROOT / "petit-kernel_amd")
    path = tmp_path / "tuned.txt"
    env = dict(os.environ, PETIT_AMD_TUNE_FILE="")
    out = subprocess.run([sys.executable, "-c", code, str(path)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    pick = int(out.stdout.strip().splitlines()[-1], 16)
    rows = [ln.split() for ln in path.read_text().splitlines() if ln and not ln.startswith("#")]
    assert rows == [["5", "3", "3072", "5120", "65", "128", f"{pick:x}"]]
    from petit_kernel import _lib
    assert _default_solution_in_subprocess({"PETIT_AMD_TUNE_FILE": str(path)}, _lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, 100, 3072, 5120) == pick


def test_tune_rows_split_on_overlap_and_merge_on_save(tmp_path):
    """A single-M row inserted into a bucket row keeps the bucket's pick for the other Ms (round 3 erased the whole bucket); petit_tune_save
    merges with what another process wrote to the same file meanwhile and replaces the file by rename (no temp file left, a lock file
    beside it); a tune file written by round 3 (b_type 8, element nibble 3) still loads, as plain MXFP4."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, ctypes as C
sys.path.insert(0, r'%s')
from petit_kernel import _lib
L = _lib.lib
at, bt, n, k = _lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, 3072, 5120
h = _lib.SolutionHints(at, bt, at, 0)
cnt = C.c_uint(0); L.petit_gemm_get_solutions(C.byref(h), 8, n, k, None, C.byref(cnt))
ids = (C.c_uint64 * cnt.value)(); L.petit_gemm_get_solutions(C.byref(h), 8, n, k, ids, C.byref(cnt))
ids = [i for i in ids if (i >> 48) & 0xF in (10, 11)]            # staged 8 / 16 rows: can serve the whole 5..8 bucket
bucket, single = ids[0], ids[1]
assert L.petit_tune_insert(C.byref(h), n, k, 5, 8, C.c_uint64(bucket)) == 0
assert L.petit_tune_insert(C.byref(h), n, k, 7, 7, C.c_uint64(single)) == 0
picks = [L.petit_gemm_default_solution(C.byref(h), m, n, k) for m in (5, 6, 7, 8)]
assert picks == [bucket, bucket, single, bucket], [hex(p) for p in picks]
# round 3's spelling of fp16 x MXFP4 with fp16-safe scales: b_type 8, element nibble 3
h16 = _lib.SolutionHints(_lib.CXX_DTYPE_FP16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_FP16, 0)
old = L.petit_gemm_default_solution(C.byref(h16), 16, 2048, 4096)
print('%%x %%x %%x' %% (bucket, single, old))
assert L.petit_tune_save(sys.argv[1].encode()) == 0
""" % (ROOT / "petit-kernel_amd")
    path = tmp_path / "shared.txt"
    path.write_text("# another rank\n5 3 9999 1024 1 1 1814411013100101\n4 8 2048 4096 9 16 181b811033100101\n")
    out = subprocess.run([sys.executable, "-c", code, str(path)], env=dict(os.environ, PETIT_AMD_TUNE_FILE=str(path)), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    bucket, single, old = (int(x, 16) for x in out.stdout.strip().splitlines()[-1].split())
    assert old == 0x181b811023100101                                  # the round-3 row was read as b_type 7 / nibble 2 and served the query
    rows = [ln.split() for ln in path.read_text().splitlines() if ln and not ln.startswith("#")]
    mine = sorted((int(r[4]), int(r[5]), int(r[6], 16)) for r in rows if r[2] == "3072")
    assert mine == [(5, 6, bucket), (7, 7, single), (8, 8, bucket)]
    assert ["5", "3", "9999", "1024", "1", "1", "1814411013100101"] in rows      # the other rank's row survived
    assert ["4", "7", "2048", "4096", "9", "16", "181b811023100101"] in rows
    assert sorted(os.listdir(tmp_path)) == ["shared.txt", "shared.txt.lock"]


def test_bench_line_stays_inside_the_drivers_record():
    """The driver keeps the last ~16 KB of bench.py's stdout: the whole JSON line must fit with room to spare (<= 12 KB with every cell of the
    plan present: round 6 added the NVFP4 native cells and the TP = 8 shard shapes), the metric's own 16 cells (bf16 x NVFP4, M in {1, 8, 16, 512}, the four Llama-3-70B linears) must END the line, and the
    bf16 x MXFP4 decode cells (the reference's only MX activation type) must be in the plan.  No GPU: cells are synthesised from the plan."""
    import importlib.util
    import json
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import benchlib as BL
    spec = importlib.util.spec_from_file_location("bench_for_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    plan = BL.bench_cell_plan()
    assert {(c["shape"], c["M"]) for c in plan if (c["a"], c["w"], c["mode"]) == ("bf16", "mx", "auto") and c["M"] <= 16} == \
        {(s, m) for s in BL.SHAPE_ORDER for m in (1, 16)}
    cells = []
    for c in plan:
        dt = f"{c['a']}x{c['w']}" + ("" if c["mode"] == "auto" else f" {c['mode']}")
        cell = {"shape": c["shape"], "M": c["M"], "dt": dt, "us": 1234.56, "us_min": 1230.01, "frac": 0.6789, "sid": "1814411013100101", "kernel": "x" * 120}
        cell["GBs" if c["M"] <= BL.HBM_BOUND_MAX_M else "TF"] = 4567 if c["M"] <= BL.HBM_BOUND_MAX_M else 1234.5
        cells.append(cell)
        if c["mode"].startswith("hipblaslt"):          # bench.py times every heuristic result and adds the fastest as its own cell
            cells.append(dict(cell, dt=dt + "_best"))
    compact = bench.compact_cells(cells)
    line = {"metric": "bf16xnvfp4_gemm_achieved_hbm_bandwidth_m1_n8192_k8192", "value": 4690.994931410796, "unit": "GB/s", "n_gpus": 1, "steps": 20,
            "warmup": 5, "ms_per_step": 0.00805405005812645, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic", "config": {"workload": "w" * 110, "parallelism": "replicas x1 (no data-path collective)", "solution": "s" * 130},
            "roofline": {"bound": "hbm", "achieved": 4690.99, "peak": 8000.0, "unit": "GB/s", "frac": 0.586, "traffic": 37980000, "traffic_source": "t" * 120},
            "host_us_per_call": {"x": "y" * 400}, "cells_method": "m" * 600, "cpu_baseline": {"value": 0.39, "unit": "GB/s", "cores": 128, "kind": "port", "sample": "s" * 200}}
    line.update(compact)
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) <= 12288, len(text)
    assert sum(len(r[2]) for r in compact["cells"]) >= len(plan) and all(len(r[2]) == len(r[3]) == len(compact["cells_m"][r[1]]) for r in compact["cells"])
    assert list(line)[-1] == "metric_cells" and len(compact["metric_cells"]) == 16
    assert {(r[0], r[1]) for r in compact["metric_cells"]} == {(s, m) for s in BL.SHAPE_ORDER for m in (1, 8, 16, 512)}
    assert all(len(r) == 6 for r in compact["metric_cells"] if r[1] <= 16)      # ... with the fraction of the 6.29 TB/s copy ceiling beside 8 TB/s


def test_native_class_default_picks():
    """solution_id -2 / -3 (PETIT_SOLUTION_AUTO_NATIVE_MXFP8 / _MXFP4): the pick comes from the class's own table, else its own
    model; it is always a native kernel of the requested activation format, needs scratch, and
    PETIT_SOLUTION_AUTO itself never resolves to one."""
    from petit_kernel import _lib
    L = _lib.lib
    rows = re.findall(r"\{(\d+), (\d+), (\d+)u, (\d+)u, (\d+)u, (\d+)u, 0x([0-9a-f]+)ull\}",
                      (ROOT / "petit-kernel_amd/csrc/tuned_native_gfx950.inc").read_text())
    assert rows
    for at, bt, n, k, lo, hi, sol in rows:
        at, bt, n, k, lo, hi, sol = int(at), int(bt), int(n), int(k), int(lo), int(hi), int(sol, 16)
        assert bt in (_lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_FP4_E2M1) and (sol >> 48) & 0xF in (9, 13)
        assert (sol >> 28) & 0xF == (2 if bt == _lib.CXX_DTYPE_MXFP4_E2M1 else 1)      # the family's element nibble: NVFP4 rows name the image kernels
        h = _lib.SolutionHints(at, bt, at, 0)
        sentinel = {6: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, 4: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, 2: _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8}[(sol >> 32) & 7]
        assert L.petit_gemm_resolve_solution(C.byref(h), row_rep_m(lo, hi), n, k, C.c_uint64(sentinel), None, C.c_uint64(1 << 40)) == sol
        assert same_kernel_split_at_most(L.petit_gemm_resolve_solution(C.byref(h), lo, n, k, C.c_uint64(sentinel), None, C.c_uint64(1 << 40)), sol)
        assert "unknown" not in _lib.describe_solution(sol)
    for at in (_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP16):
        h = _lib.SolutionHints(at, _lib.CXX_DTYPE_MXFP4_E2M1, at, 0)
        for (m, n, k) in [(512, 5120, 13824), (64, 96, 512), (2048, 57344, 8192), (300, 4096, 768), (17, 32, 256)]:   # unseen shapes, every span size
            exact = L.petit_gemm_default_solution(C.byref(h), m, n, k)
            assert exact and (exact >> 48) & 0xF not in (9, 13)
            for sentinel, code in ((_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, 2), (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, 4), (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, 6)):
                sid = L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(sentinel), None, C.c_uint64(1 << 40))
                assert sid and (sid >> 48) & 0xF in (9, 13) and (sid >> 32) & 7 == code, (m, n, k, hex(sid))
                need = L.petit_gemm_workspace_bytes(C.byref(h), m, n, k, C.c_uint64(sentinel))
                assert need >= m * k // 2
                # scratch that covers the quantised activations but no K-split slabs: the same kernel, unsplit
                small = L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(sentinel), None, C.c_uint64(_lib.lib.petit_native_workspace_bytes(m, k)))
                assert small and (small >> 60) == 1 and (small ^ sid) & ~(0xF << 60) == 0
                assert L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(sentinel), None, C.c_uint64(0)) == 0
        # NVFP4 weights (round 6): the class exists there too -- on the MFMA-native image of the weights (test_nv6_entry_points_validate_without_a_gpu);
        # its kernels carry the NVFP4 family's element nibble, and PETIT_SOLUTION_AUTO never resolves to one
        hn = _lib.SolutionHints(at, _lib.CXX_DTYPE_FP4_E2M1, at, 0)
        for (m, n, k) in [(512, 8192, 8192), (300, 4096, 768), (64, 96, 512)]:
            sid = L.petit_gemm_resolve_solution(C.byref(hn), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4), None, C.c_uint64(1 << 40))
            assert sid and (sid >> 48) & 0xF == 13 and (sid >> 28) & 0xF == 1 and (sid >> 32) & 7 == 6, hex(sid)
            assert L.petit_gemm_workspace_bytes(C.byref(hn), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8)) >= m * k // 2
            assert (L.petit_gemm_default_solution(C.byref(hn), m, n, k) >> 48) & 0xF not in (9, 13)


def test_process_wide_default_class_for_mxfp4_weights():
    """petit_set_mxfp4_default_class (= $PETIT_AMD_MXFP4_ACTIVATIONS): PETIT_SOLUTION_AUTO on MXFP4 weights resolves inside the named native class
    for m >= 64 when the scratch covers it, nowhere else; off by default; needs no GPU to decide."""
    from petit_kernel import _lib
    L = _lib.lib
    mx = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    nv = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    auto = C.c_uint64(_lib.PETIT_SOLUTION_AUTO)
    kind = lambda sid: (sid >> 48) & 0xF
    assert L.petit_get_mxfp4_default_class() == 0
    exact = {m: L.petit_gemm_default_solution(C.byref(mx), m, 8192, 8192) for m in (16, 512)}
    assert all(kind(s) not in (9, 13) for s in exact.values())
    assert L.petit_set_mxfp4_default_class(5) == _lib.PETIT_ERROR_BAD_ARGUMENT
    try:
        for fmt, code in ((8, 2), (6, 4), (4, 6)):
            assert L.petit_set_mxfp4_default_class(fmt) == 0 and L.petit_get_mxfp4_default_class() == fmt
            sid = L.petit_gemm_default_solution(C.byref(mx), 512, 8192, 8192)
            assert kind(sid) in (9, 13) and (sid >> 32) & 7 == code, hex(sid)
            assert L.petit_gemm_workspace_bytes(C.byref(mx), 512, 8192, 8192, auto) >= 512 * 8192 // 2
            # no scratch -> the exact default, as before; small M and NVFP4 weights: never
            assert L.petit_gemm_resolve_solution(C.byref(mx), 512, 8192, 8192, auto, None, C.c_uint64(0)) == exact[512] or \
                kind(L.petit_gemm_resolve_solution(C.byref(mx), 512, 8192, 8192, auto, None, C.c_uint64(0))) not in (9, 13)
            assert L.petit_gemm_default_solution(C.byref(mx), 16, 8192, 8192) == exact[16]
            assert kind(L.petit_gemm_default_solution(C.byref(nv), 512, 8192, 8192)) not in (9, 13)
    finally:
        assert L.petit_set_mxfp4_default_class(0) == 0
    assert L.petit_gemm_default_solution(C.byref(mx), 512, 8192, 8192) == exact[512]


def test_tune_params_struct_matches_the_header():
    from petit_kernel import _lib
    text = (ROOT / "include/petit_amd.h").read_text()
    body = text[text.index("typedef struct petit_tune_params {"):text.index("} petit_tune_params;")]
    fields = re.findall(r"^\s+(?:const void \*const \*|u?int(?:32|64)_t |float )\s*(\w+(?:, \w+)*);", body, flags=re.M)
    names = [n.strip() for f in fields for n in f.split(",")]
    assert names == [f[0] for f in _lib.TuneParams._fields_]
    assert C.sizeof(_lib.TuneParams) == 64


def test_new_entry_points_validate_before_they_launch():
    """Argument checks of the round-3 entry points that need no GPU: every refusal happens before anything is enqueued."""
    from petit_kernel import _lib
    L = _lib.lib
    fake = C.c_void_p(4096)                                   # never dereferenced: the checks come first
    h_nv = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    h_mx = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    # grouped launch
    mem = (_lib.GroupMember * 9)(*[_lib.GroupMember(4096, 4096, 4096, 4096, None, 256, 0) for _ in range(9)])
    auto = C.c_uint64(_lib.PETIT_SOLUTION_AUTO)
    assert L.petit_gemm_fp4_fp16_grouped(mem, 9, fake, 1, 1024, C.byref(h_nv), auto, None) == _lib.PETIT_ERROR_BAD_ARGUMENT      # > 8 members
    assert L.petit_gemm_fp4_fp16_grouped(mem, 3, fake, 17, 1024, C.byref(h_nv), auto, None) == _lib.PETIT_ERROR_KERNEL_SHAPE      # not the decode regime
    assert L.petit_gemm_fp4_fp16_grouped(mem, 3, fake, 1, 1000, C.byref(h_nv), auto, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE      # k % 256
    assert L.petit_gemm_fp4_fp16_grouped(mem, 0, fake, 1, 1024, C.byref(h_nv), auto, None) == 0                                   # empty group: nothing to do
    bad = (_lib.GroupMember * 1)(_lib.GroupMember(4096, None, 4096, 4096, None, 256, 0))
    assert L.petit_gemm_fp4_fp16_grouped(bad, 1, fake, 1, 1024, C.byref(h_nv), auto, None) == _lib.PETIT_ERROR_BAD_ARGUMENT
    odd = (_lib.GroupMember * 1)(_lib.GroupMember(4096, 4096, 4096, 4096, None, 250, 0))
    assert L.petit_gemm_fp4_fp16_grouped(odd, 1, fake, 1, 1024, C.byref(h_nv), auto, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE      # n % 16
    # the native entry point
    na = _lib.NativeArgs(C.sizeof(_lib.NativeArgs), 4, 0, 0)
    call = lambda hints, sid, nargs, n=512, k=1024, epi=None, c=fake, a=fake: L.petit_gemm_mxfp4_native(
        c, a, fake, fake, fake, 64, n, k, C.byref(hints), C.c_uint64(sid), epi, C.byref(nargs) if nargs is not None else None, None, C.c_uint64(0), None)
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO, na) == _lib.PETIT_ERROR_KERNEL_SHAPE                      # plain AUTO never enters the class
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, na) == _lib.PETIT_ERROR_KERNEL_SHAPE         # MXFP4-quantised input, MXFP8 class
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, _lib.NativeArgs(8, 4, 0, 0)) == _lib.PETIT_ERROR_BAD_ARGUMENT    # struct size
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, _lib.NativeArgs(16, 5, 0, 0)) == _lib.PETIT_ERROR_BAD_ARGUMENT   # unknown format
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, _lib.NativeArgs(16, 0, 4, 0)) == _lib.PETIT_ERROR_BAD_ARGUMENT   # quantised output without SiLU-mul
    epi = _lib.Epilogue(None, 1, 0)
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, _lib.NativeArgs(16, 0, 4, 0), n=768, epi=C.byref(epi)) == _lib.PETIT_ERROR_PROBLEM_SHAPE  # n % 512
    assert call(h_mx, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, na, a=C.c_void_p(4100)) == _lib.PETIT_ERROR_BAD_ARGUMENT         # misaligned quantised input
    # sizes of the quantised-activation format
    assert L.petit_quantized_activation_bytes(512, 8192, 4) == 512 * 8192 // 2 + 512 * 8192 // 32
    assert L.petit_quantized_activation_bytes(512, 8192, 8) == 512 * 8192 + 512 * 8192 // 32 == L.petit_native_workspace_bytes(512, 8192)
    assert L.petit_quantized_activation_bytes(512, 8192, 6) == 512 * 8192 * 3 // 4 + 512 * 8192 // 32      # MXFP6: 24 bytes per 32-k block
    assert L.petit_quantized_activation_bytes(512, 8192, 5) == 0
    assert L.petit_quantize_activations(fake, fake, 4, 1000, _lib.CXX_DTYPE_BF16, 4, None) == _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert L.petit_quantize_activations(fake, fake, 4, 1024, 3, 4, None) == _lib.PETIT_ERROR_KERNEL_SHAPE                   # not a 16-bit activation type
    assert L.petit_quantize_activations(None, fake, 4, 1024, _lib.CXX_DTYPE_BF16, 4, None) == _lib.PETIT_ERROR_BAD_ARGUMENT
    # the scratch a pipeline call needs: with quantised input only the slabs of a K split remain
    full = L.petit_gemm_native_workspace_bytes(C.byref(h_mx), 512, 8192, 8192, C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4), None, None)
    pre = L.petit_gemm_native_workspace_bytes(C.byref(h_mx), 512, 8192, 8192, C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4), None, C.byref(na))
    assert full >= 512 * 8192 // 2 and pre < 512 * 8192 // 2
    # the tuner
    tp = _lib.TuneParams(8, 0, 1, 0, None, None, 0, 0, 0.0, 0, 0, 0, 0)
    best, us = C.c_uint64(0), C.c_float(0)
    assert L.petit_gemm_tune(fake, fake, fake, 16, 512, 1024, C.byref(h_nv), C.byref(tp), None, C.c_uint64(0), None, C.byref(best), C.byref(us)) == _lib.PETIT_ERROR_BAD_ARGUMENT
    tp = _lib.TuneParams(C.sizeof(_lib.TuneParams), 3, 1, 0, None, None, 0, 0, 0.0, 0, 0, 0, 0)                              # unknown class
    assert L.petit_gemm_tune(fake, fake, fake, 16, 512, 1024, C.byref(h_nv), C.byref(tp), None, C.c_uint64(0), None, C.byref(best), C.byref(us)) == _lib.PETIT_ERROR_BAD_ARGUMENT


# --- round 5: M buckets above 512, the K-split guard, the ranges the entry points accept ---------------------------------------------

def _table_rows(name):
    text = (ROOT / "petit-kernel_amd" / "csrc" / name).read_text()
    return [(int(at), int(bt), int(n), int(k), int(lo), int(hi), int(sol, 16))
            for at, bt, n, k, lo, hi, sol in re.findall(r"\{(\d+), (\d+), (\d+)u, (\d+)u, (\d+)u, (\d+)u, 0x([0-9a-f]+)ull\}", text)]


def test_table_buckets_and_the_split_guard():
    """the open-ended bucket [257, 1 << 20] is gone -- prefill has its own rows (513-1024, 1025-4096, 4097+) -- and no row of
    either table names a cross-workgroup K split that the library's guard (csrc/api.hip guarded_splitk, restated in tools/split_buckets.py) would take
    away at the M the row stands for: no split once the unsplit grid has >= 2 workgroups per CU, slabs never larger than the operands."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import split_buckets as SB
    from petit_kernel import _lib
    for name, native in (("tuned_gfx950.inc", False), ("tuned_native_gfx950.inc", True)):
        rows = _table_rows(name)
        per_shape = {}
        for at, bt, n, k, lo, hi, sol in rows:
            per_shape.setdefault((at, bt, n, k, (sol >> 32) & 7 if native else 0), []).append((lo, hi))
            m = row_rep_m(lo, hi)
            sk = (sol >> 60) & 0xF
            assert SB.guarded_splitk(sol, m, n, k) == sk, (name, n, k, lo, hi, hex(sol))
            if sk > 1:
                bm, bn = SB.tile(sol)
                assert -(-m // bm) * -(-n // bn) < 512
                group = 16 if bt == _lib.CXX_DTYPE_FP4_E2M1 else 32
                assert sk * m * n * 4 <= n * k // 2 + n * k // group + 2 * m * k + 2 * m * n
        for key, ranges in per_shape.items():
            ranges.sort()
            assert (257, 1 << 20) not in ranges, key
            if ranges[-1][1] == 1 << 20:   # (every shape of the generated tables reaches the last bucket)
                assert ranges[-1][0] == 4097 and (1025, 4096) in ranges and (513, 1024) in ranges and (257, 512) in ranges, key
    # a prefill chunk of the largest shape: whatever the row says, AUTO asks for no scratch beyond what the operands weigh -- and none at all here
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    for (n, k) in [(57344, 8192), (8192, 28672), (10240, 8192), (8192, 8192), (1280, 8192)]:
        for m in (1024, 2084, 4314, 16375):
            assert _lib.lib.petit_gemm_workspace_bytes(C.byref(h), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)) <= n * k // 2 + n * k // 16 + 2 * m * (n + k), (m, n, k)
        assert _lib.lib.petit_gemm_workspace_bytes(C.byref(h), 16375, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)) == 0, (n, k)
    # and a run-time row measured at a small M is guarded the same way when a larger M of its range is asked for
    code = r"""
import sys, ctypes as C
sys.path.insert(0, %r)
from petit_kernel import _lib
L = _lib.lib
h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
cnt = C.c_uint(0)
L.petit_gemm_get_solutions(C.byref(h), 300, 4352, 8192, None, C.byref(cnt))
ids = (C.c_uint64 * cnt.value)()
L.petit_gemm_get_solutions(C.byref(h), 300, 4352, 8192, ids, C.byref(cnt))
tiled = next(i for i in ids if (i >> 48) & 0xF == 8 and (i & 0xFF) == 4)       # a 64-row tiled kernel
row = (tiled & ~(0xF << 60)) | (2 << 60)
assert L.petit_tune_insert(C.byref(h), 4352, 8192, 257, 1 << 20, C.c_uint64(row)) == 0
print(hex(L.petit_gemm_default_solution(C.byref(h), 300, 4352, 8192)), hex(L.petit_gemm_default_solution(C.byref(h), 16375, 4352, 8192)), hex(row))
""" % str(ROOT / "petit-kernel_amd")
    import subprocess
    small, large, row = (int(x, 16) for x in subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.split())
    assert small == row and large == (row & ~(0xF << 60)) | (1 << 60)


def test_raster_maps_every_workgroup_to_its_own_tile():
    """petit_raster_tile = csrc/device_common.hpp tile_of_linear, the function the large-M kernels call with their blockIdx: for any grid and any band height
    (0 = whole columns, bands that do not divide the m-tile count, bands taller than the grid) the map workgroup -> C tile is a bijection onto the grid; and
    with a band of 4 the 32 workgroups an XCD runs at a time (linear ids b, b + 8, ...: one XCD) cover at most 4 m-tiles x 9 n-tiles -- the point of the band."""
    from petit_kernel import _lib
    bn, bm = C.c_uint(0), C.c_uint(0)

    def tile(nx, ny, band, b):
        _lib.lib.petit_raster_tile(nx, ny, band, b, C.byref(bn), C.byref(bm))
        return bn.value, bm.value
    for nx in (1, 3, 7, 32, 40, 224):
        for ny in (1, 2, 5, 9, 17, 34, 128):
            for band in (0, 1, 2, 3, 4, 8, 32, 200):
                seen = {tile(nx, ny, band, b) for b in range(nx * ny)}
                assert len(seen) == nx * ny and all(x < nx and y < ny for x, y in seen), (nx, ny, band)
    for nx, ny in ((224, 128), (32, 128), (40, 17)):
        for start in (0, 8 * 32 * 5, 8 * 32 * 11):
            if start + 8 * 32 > nx * ny:
                continue
            for xcd in range(8):
                tiles = [tile(nx, ny, 4, start + xcd + 8 * i) for i in range(32)]
                assert len({y for _, y in tiles}) <= 4 and len({x for x, _ in tiles}) <= 9, (nx, ny, start, xcd)
                whole = [tile(nx, ny, 0, start + xcd + 8 * i) for i in range(32)]
                assert ny < 32 or len({x for x, _ in whole}) <= 2    # whole columns: one W panel, 32 A panels -- what rounds 2-4 did


def test_no_prefill_row_names_a_weight_streaming_kernel():
    """Round 5 found 33 fp16 x MXFP4 rows of the prefill buckets naming the streaming REFERENCE kernel (ten times slower than the tiled ones at M = 8192): the
    tuner's output check demanded that inf agree, and fp16 outputs of its synthetic long-K problems sit near 65504, so every kernel with another summation order
    than the reference was rejected (csrc/tune.hip compare_outputs_kernel now saturates).  The table's invariant since: above M = 256 every row is a kernel
    with a tile grid -- tiled / wide32 / shared-unpack (codes 8, 12) or the batched-decode kernel (code 0, warp_partition_m 2)."""
    text = (ROOT / "petit-kernel_amd" / "csrc" / "tuned_gfx950.inc").read_text()
    rows = re.findall(r"^\{(\d+), (\d+), (\d+)u, (\d+)u, (\d+)u, (\d+)u, 0x([0-9a-f]+)ull\},$", text, re.M)
    big = [(int(lo), int(sid, 16)) for _, _, _, _, lo, _, sid in rows if int(lo) >= 257]
    assert len(big) >= 4 * 92 * 4
    for lo, sid in big:
        code, wm = (sid >> 48) & 0xF, (sid >> 36) & 0xF
        assert code in (8, 12) or (code == 0 and wm == 2), (lo, hex(sid))


def test_ragged_prefill_m_is_planned_as_bulk_plus_tail():
    """petit_gemm_auto_row_split (csrc/api.hip plan_row_split): a default-pick call whose tile grid ends a little past a whole number of rounds runs as two
    launches.  The plan is host arithmetic: never at M <= 512, the bulk is a whole number of 16-row tiles and shorter than M, the bulk itself is not split
    again, the scratch the library asks for covers both parts, and the Llama-70B `down` shape at the reference's ragged M = 2084
    (tools/benchmarks/matmul.py) is one of the cases it fires on (17 m-tiles of 128 rows x 32 n-tiles = 2.1 rounds of 256 CUs)."""
    from petit_kernel import _lib
    fired = 0
    for at in (_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP16):
        for bt in (_lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1):
            h = _lib.SolutionHints(at, bt, at, 0)
            for n, k in ((8192, 8192), (8192, 28672), (10240, 8192), (57344, 8192), (4096, 4096), (3072, 8192)):
                for m in (1, 16, 300, 512, 520, 600, 777, 1024, 1100, 1500, 2048, 2084, 2200, 3000, 4314, 8192, 16375):
                    m1 = _lib.lib.petit_gemm_auto_row_split(C.byref(h), m, n, k, None)
                    if m <= 512:
                        assert m1 == 0
                    if not m1:
                        continue
                    fired += 1
                    # (the tail is at most one round's worth of m-tiles: on a narrow N with a wide tile -- 3072 = 9.6 tiles of 320 columns -- that is 1114 of 4314 rows)
                    assert 0 < m1 < m and m1 % 16 == 0 and m - m1 < m1 and m - m1 <= 3584, (at, bt, n, k, m, m1)
                    assert _lib.lib.petit_gemm_auto_row_split(C.byref(h), m1, n, k, None) == 0
                    ws = lambda mm: int(_lib.lib.petit_gemm_workspace_bytes(C.byref(h), mm, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)))
                    assert ws(m) == max(ws(m1), ws(m - m1))
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    assert _lib.lib.petit_gemm_auto_row_split(C.byref(h), 2084, 8192, 28672, None) == 2048
    assert fired >= 8
    # the process-wide MXFP4 default class: AUTO at a ragged M runs bulk + tail in the class, and the queries describe that call -- the row split,
    # and scratch that covers both parts and the class's own pick (the class is taken only when the call's scratch covers it)
    L = _lib.lib
    prev = L.petit_get_mxfp4_default_class()
    L.petit_set_mxfp4_default_class(8)
    try:
        hm = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
        m, n, k = 2084, 8192, 8192
        m1 = L.petit_gemm_auto_row_split(C.byref(hm), m, n, k, None)
        assert 0 < m1 < m and m - m1 <= 128 and m1 % 16 == 0, m1
        assert L.petit_gemm_row_split(C.byref(hm), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None) == m1
        assert L.petit_gemm_auto_row_split(C.byref(hm), m1, n, k, None) == 0
        ws = lambda mm: int(L.petit_gemm_workspace_bytes(C.byref(hm), mm, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)))
        assert ws(m) >= max(ws(m1), ws(m - m1)) > 0
        sid = int(L.petit_gemm_resolve_solution(C.byref(hm), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None, C.c_uint64(ws(m))))
        assert (sid >> 48) & 0xF == 13, hex(sid)   # (the whole problem's kernel, for that scratch: the class's)
    finally:
        L.petit_set_mxfp4_default_class(prev)


def test_problem_ranges_are_refused_not_wrapped():
    """M beyond the tables' last bucket, and a native-class problem whose quantised activations outgrow one 32-bit buffer descriptor, return
    PETIT_ERROR_PROBLEM_SHAPE before anything is launched (no GPU here: a launch would fail differently)."""
    from petit_kernel import _lib
    L = _lib.lib
    buf = (C.c_uint * 64)()
    p = C.cast(buf, C.c_void_p)
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    assert L.petit_gemm_fp4_fp16_grid(p, p, p, p, p, (1 << 20) + 1, 8192, 8192, C.byref(h), C.c_uint64(_lib.PETIT_SOLUTION_AUTO), None) == 1
    hm = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_MXFP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    ws = C.c_void_p(256)
    for sentinel in (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4):
        assert L.petit_gemm_mxfp4_native(p, p, p, p, p, 65535, 8192, 66560, C.byref(hm), C.c_uint64(sentinel), None, None, ws, C.c_uint64(1 << 40), None) == 1
        assert L.petit_gemm_mxfp4_native(p, p, p, p, p, 65536, 8192, 8192, C.byref(hm), C.c_uint64(sentinel), None, None, ws, C.c_uint64(1 << 40), None) == 1
        # ... and the queries agree with the launcher (VERDICT r05 hygiene 8): no kernel, no scratch for a problem it refuses
        assert L.petit_gemm_resolve_solution(C.byref(hm), 65536, 8192, 8192, C.c_uint64(sentinel), None, C.c_uint64(1 << 40)) == 0
        assert L.petit_gemm_resolve_solution(C.byref(hm), 65535, 8192, 66560, C.c_uint64(sentinel), None, C.c_uint64(1 << 40)) == 0
        assert L.petit_gemm_resolve_solution(C.byref(hm), 512, 8192, 8192, C.c_uint64(sentinel), None, C.c_uint64(1 << 40)) != 0
    # the enumeration and the default pick answer "nothing" exactly where the launcher refuses (M > 2^20) or has nothing to do (m, n or k = 0) --
    # the reference's enumeration filters by what its kernels accept (algo_chooser.cc:14-62)
    cnt = C.c_uint(0)
    for hints in (h, hm):
        for (m, n, k) in (((1 << 20) + 1, 8192, 8192), (1 << 21, 8192, 8192), (16, 0, 8192), (16, 8192, 0), (0, 8192, 8192)):
            assert L.petit_gemm_default_solution(C.byref(hints), m, n, k) == 0, (m, n, k)
            assert L.petit_gemm_get_solutions(C.byref(hints), m, n, k, None, C.byref(cnt)) == 0 and cnt.value == 0, (m, n, k)
            assert L.petit_gemm_workspace_bytes(C.byref(hints), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO)) == 0
            assert L.petit_gemm_auto_row_split(C.byref(hints), m, n, k, None) == 0
        assert L.petit_gemm_default_solution(C.byref(hints), 1 << 20, 8192, 8192) != 0
        assert L.petit_gemm_get_solutions(C.byref(hints), 1 << 20, 8192, 8192, None, C.byref(cnt)) == 0 and cnt.value > 0


def test_native_silu_mul_without_slab_scratch_names_a_kernel_that_applies_it():
    """the native table has rows like the 64 x 320 kernel (five n-tiles per wave) x K split 4 for N = 1280, K = 8192, M >= 257.
    With SiLU-mul such a row is fine while the split's reduce pass applies the activation -- but when the caller's scratch covers the quantised
    activations only, the unsplit fallback must not keep a kernel whose own epilogue cannot (odd n-tiles per wave): the resolved kernel has an even
    count, whatever the scratch."""
    from petit_kernel import _lib
    L = _lib.lib
    epi = _lib.Epilogue(None, 1, 0)
    for at in (_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP16):
        h = _lib.SolutionHints(at, _lib.CXX_DTYPE_MXFP4_E2M1, at, 0)
        for sentinel in (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, _lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4):
            for (m, n, k) in [(512, 1280, 8192), (300, 1280, 8192), (512, 2560, 8192), (1024, 1280, 8192), (512, 7168, 2048)]:
                for ws in (1 << 40, L.petit_native_workspace_bytes(m, k)):
                    sid = L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(sentinel), C.byref(epi), C.c_uint64(ws))
                    assert sid, (m, n, k, ws)
                    ntw, split = (sid >> 52) & 0xF, sid >> 60
                    assert split > 1 or ntw % 2 == 0, (m, n, k, ws, hex(sid), _lib.describe_solution(sid))
                    if ws < 1 << 40:
                        assert split == 1 and ntw % 2 == 0, (hex(sid), _lib.describe_solution(sid))


def test_collapsed_k_split_with_silu_mul_is_decided_in_the_plan():
    """A K of one span cannot be split: a split nibble of 2 gives one slice and no reduce pass, so SiLU-mul -- which rides on the reduce pass of a real
    split -- is the kernel's own epilogue's job.  The plan knows the launch geometry, so petit_gemm_resolve_solution answers as the launcher will: an
    explicit id resolves exactly when its kernel can apply the epilogue (an even number of n-tiles per wave, and not the LDS-shared kernel, whose
    epilogue is plain / bias only), and PETIT_SOLUTION_AUTO names such a kernel.  k = 256 / 512 / 1024 are one span at span sizes 2 / 4 / 8."""
    from petit_kernel import _lib
    L = _lib.lib
    epi = _lib.Epilogue(None, 1, 0)
    applies = lambda sid: ((sid >> 52) & 0xF) % 2 == 0 and not ((sid >> 48) & 0xF == 12 and (sid >> 36) & 0xF == 5)
    seen = set()
    for at in (_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP16):
        for bt in (_lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_MXFP4_E2M1):
            h = _lib.SolutionHints(at, bt, at, 0)
            for k in (256, 512, 1024):
                for n in (64, 256):
                    for m in (40, 300):
                        cnt = C.c_uint(0)
                        L.petit_gemm_get_solutions(C.byref(h), m, n, k, None, C.byref(cnt))
                        buf = (C.c_uint64 * cnt.value)()
                        L.petit_gemm_get_solutions(C.byref(h), m, n, k, buf, C.byref(cnt))
                        for sid in buf[:cnt.value]:
                            kind, wm = (sid >> 48) & 0xF, (sid >> 36) & 0xF
                            if not (kind == 8 or kind == 12 or (kind == 0 and wm == 2)):
                                continue
                            seen.add((kind, wm == 5, applies(sid)))
                            split2 = (sid & ~(0xF << 60)) | (2 << 60)
                            got = L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(split2), C.byref(epi), C.c_uint64(1 << 40))
                            assert (got != 0) == applies(sid), (m, n, k, hex(sid), hex(got), _lib.describe_solution(sid))
                        auto = L.petit_gemm_resolve_solution(C.byref(h), m, n, k, C.c_uint64(_lib.PETIT_SOLUTION_AUTO), C.byref(epi), C.c_uint64(1 << 40))
                        assert auto and applies(auto), (m, n, k, hex(auto), _lib.describe_solution(auto))
    # every kind met, kernels that apply the epilogue and kernels that do not
    assert {(8, False, True), (8, False, False), (12, False, True), (12, True, False), (0, False, True), (0, False, False)} <= seen, seen


# --- the MFMA-native image of NVFP4 weights (csrc/nvnative.hip): the host twin against its numpy statement ------------------------

def _checkpoint_like_nvfp4(n, k, seed):
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import quantize_weights as QW
    q, s, ws2 = QW.quantize_nvfp4(QW.synthetic_weights(n, k, seed=seed))
    return q, s, ws2


@pytest.mark.parametrize("n,k,kind", [(32, 256, "uniform"), (48, 512, "uniform"), (64, 1024, "checkpoint"), (80, 768, "checkpoint"), (128, 2048, "checkpoint")])
def test_nv6_image_host_twin_matches_its_statement(n, k, kind):
    """petit_nvfp4_native_image_host + _dequant_host against oracle.nv6_reencode (E = floor(log2 max |fp4 x e4m3|) - 2, elements RNE to e2m3): every
    value identical; the re-rounding stays inside the stated per-element bound (include/petit_amd.h) and moves checkpoint-like weights by ~2 % rms."""
    import petit_kernel
    rng = np.random.default_rng(n + k)
    if kind == "uniform":
        q = rng.integers(0, 256, (n, k // 2), dtype=np.uint8)
        s = rng.integers(0, 0x7F, (n, k // 16), dtype=np.uint8)            # any non-NaN e4m3 byte, subnormals and zero included
        s[rng.random(s.shape) < 0.05] |= 0x80                              # a few negative scales
    else:
        q, s, _ = _checkpoint_like_nvfp4(n, k, n + k)
    b = petit_kernel.offline.repack_nvfp4_cpu(torch.from_numpy(q.copy()).view(torch.int32), n, k)
    sp = petit_kernel.offline.process_nvfp4_scales_cpu(torch.from_numpy(s.copy()).view(torch.float8_e4m3fn), n, k)
    image = petit_kernel.offline.nvfp4_native_image_cpu(b, sp, n, k)
    assert image.numel() == ((n + 31) // 32) * (k // 128) * (3072 + 128)
    got = petit_kernel.offline.nvfp4_native_image_dequant_cpu(image, n, k).numpy()
    want, sbytes = O.nv6_reencode(q, s)
    assert np.array_equal(got, want)
    exact = O.dequant_nvfp4(q, s).astype(np.float64)
    scale = np.repeat(np.ldexp(1.0, sbytes.astype(np.int64) - 127), 32, axis=1)
    assert (np.abs(got - exact) <= np.maximum(2.0 ** -4 * np.abs(exact), scale * 2.0 ** -4)).all()
    if kind == "checkpoint":
        rel = np.sqrt(np.mean((got - exact) ** 2) / np.mean(exact ** 2))
        assert rel < 0.03, rel


def test_nv6_entry_points_validate_without_a_gpu():
    from petit_kernel import _lib
    L = _lib.lib
    assert L.petit_nvfp4_native_image_bytes(8192, 8192) == 8192 * 8192 * 3 // 4 + 8192 * 8192 // 32
    assert L.petit_nvfp4_native_image_bytes(200, 64) == 0 and L.petit_nvfp4_native_image_bytes(256, 24) == 0
    assert L.petit_nvfp4_native_image_bytes(256, 48) == 2 * 2 * 3200          # N = 48: two n32-blocks, the second half empty
    buf = (C.c_uint8 * 4096)()
    assert L.petit_nvfp4_native_image_host(None, buf, buf, 256, 32) == _lib.PETIT_ERROR_BAD_ARGUMENT
    assert L.petit_nvfp4_native_image_host(buf, buf, buf, 200, 32) == _lib.PETIT_ERROR_PROBLEM_SHAPE
    assert L.petit_nvfp4_native_attach(None, None) == _lib.PETIT_ERROR_BAD_ARGUMENT
    assert L.petit_nvfp4_native_attach(C.addressof(buf), 256 * 7) == 0                      # (pointers are only remembered)
    assert L.petit_nvfp4_native_attached(C.addressof(buf)) == 256 * 7
    assert L.petit_nvfp4_native_attach(C.addressof(buf), 3) == _lib.PETIT_ERROR_BAD_ARGUMENT  # images are 256-byte aligned
    assert L.petit_nvfp4_native_attach(C.addressof(buf), None) == 0
    assert L.petit_nvfp4_native_attached(C.addressof(buf)) is None
    # the native class on NVFP4 weights: sentinels resolve to kernels of the NVFP4 family (element_b nibble 1) with the scratch of the class
    h = _lib.SolutionHints(_lib.CXX_DTYPE_BF16, _lib.CXX_DTYPE_FP4_E2M1, _lib.CXX_DTYPE_BF16, 0)
    for sentinel, code in ((_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8, 2), (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP6, 4), (_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP4, 6)):
        sid = L.petit_gemm_resolve_solution(C.byref(h), 1024, 8192, 8192, C.c_uint64(sentinel), None, C.c_uint64(1 << 40))
        assert sid and (sid >> 48) & 0xF == 13 and (sid >> 28) & 0xF == 1 and (sid >> 32) & 7 == code, hex(sid)
        assert L.petit_gemm_workspace_bytes(C.byref(h), 1024, 8192, 8192, C.c_uint64(sentinel)) >= 1024 * 8192 // 2
    # ... and a call without an image is refused before anything is launched (no GPU needed to see it)
    rc = L.petit_gemm_fp4_fp16_grid_ws(C.addressof(buf), C.addressof(buf), C.addressof(buf), C.addressof(buf), C.addressof(buf), 64, 64, 256, C.byref(h),
                                       C.c_uint64(_lib.PETIT_SOLUTION_AUTO_NATIVE_MXFP8), None, None, 0, None)
    assert rc == _lib.PETIT_ERROR_KERNEL_SHAPE


def test_reference_benchmark_list_is_restated_whole():
    """tools/reference_list_sweep.py restates the reference's benchmark problems by shape family (tools/benchmarks/matmul.py:8-117): 104 distinct (m, n, k), the
    reference's M values, every one inside the library's range and with a default pick; the same multiset as the reference's list, stored in
    tests/golden/reference_matmul_problems.npz (make_golden.py)."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import reference_list_sweep as RL
    probs = RL.problems()
    assert len(probs) == 104 and len(set(probs)) == 104
    assert sorted({m for m, _, _ in probs}) == [15, 16, 44, 256, 512, 566, 582, 611, 874, 932, 1003, 1324, 1340, 1466, 1906, 2084, 4314, 14437, 15961, 16375]
    assert all(n % 16 == 0 and k % 256 == 0 for _, n, k in probs)
    listed = [tuple(int(x) for x in t) for t in np.load(ROOT / "tests" / "golden" / "reference_matmul_problems.npz")["mnk"]]
    assert sorted(listed) == sorted(probs)

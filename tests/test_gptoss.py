"""petit_kernel.gptoss: the load-time helper for gpt-oss's expert layout (interleaved gate / up rows, 2880 -> 3072 padding, biases) and its
forward on the fused and the native MoE layer, against a float64 statement of the gpt-oss expert block built from the checkpoint tensors
as stored (the oracle's dequant of the raw blocks, interleaved rows, biases, clamps, the (up + 1) term, router weights on down + bias).

Bounds of the layer tests are the existing layers' own: rms error / output rms <= 1e-2 against the f64 layer and one 16-bit ulp between
fp4_moe_fused and fp4_moe (tests/test_moe_fused.py); the native layer against the exact fused layer on the same weights within 0.1
(mxfp8, mxfp6) / 0.4 (mxfp4) relative rms (tests/test_moe_native.py), hence within that plus 1e-2 of the f64 layer (triangle inequality).
"""
import numpy as np
import pytest
import torch

from oracle import cdna4_layout as LY
from oracle import oracle as O
from test_moe import _routing

DEV = "cuda"
ALPHA, LIMIT = 1.702, 7.0


def synth_checkpoint(E, H, I, seed, band=(122, 128)):
    """The six expert tensors of one MoE block as a gpt-oss checkpoint stores them, from known random codes, scales and biases."""
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    return dict(
        gate_up_blocks=t(rng.integers(0, 256, (E, 2 * I, H // 32, 16), dtype=np.uint8)),
        gate_up_scales=t(rng.integers(band[0], band[1], (E, 2 * I, H // 32), dtype=np.uint8)),
        gate_up_bias=t(rng.standard_normal((E, 2 * I)).astype(np.float32) * 0.5).bfloat16(),
        down_blocks=t(rng.integers(0, 256, (E, H, I // 32, 16), dtype=np.uint8)),
        down_scales=t(rng.integers(band[0], band[1], (E, H, I // 32), dtype=np.uint8)),
        down_bias=t(rng.standard_normal((E, H)).astype(np.float32) * 0.5).bfloat16())


def _dq(blocks_e, scales_e):
    """one expert's raw blocks [rows, K / 32, 16] + scales [rows, K / 32] -> f32 [rows, K] (the oracle's MXFP4 dequant)."""
    rows = blocks_e.shape[0]
    return O.dequant_mxfp4(blocks_e.reshape(rows, -1).numpy(), scales_e.numpy())


def gptoss_ref(ck, x, topk_w, topk_ids):
    """float64 gpt-oss expert block on the checkpoint's own layout, for the routed experts only; ids outside [0, E) contribute nothing."""
    E = ck["gate_up_blocks"].shape[0]
    xf = x.float().numpy().astype(np.float64)
    out = np.zeros((xf.shape[0], ck["down_blocks"].shape[1]))
    for e in np.unique(topk_ids):
        if e < 0 or e >= E:
            continue
        tok, slot = np.nonzero(topk_ids == e)
        y1 = xf[tok] @ _dq(ck["gate_up_blocks"][e], ck["gate_up_scales"][e]).astype(np.float64).T + ck["gate_up_bias"][e].float().numpy().astype(np.float64)
        g = np.minimum(y1[:, 0::2], LIMIT)
        u = np.clip(y1[:, 1::2], -LIMIT, LIMIT)
        h = g / (1.0 + np.exp(-ALPHA * g)) * (u + 1.0)
        y2 = h @ _dq(ck["down_blocks"][e], ck["down_scales"][e]).astype(np.float64).T + ck["down_bias"][e].float().numpy().astype(np.float64)
        np.add.at(out, tok, y2 * topk_w[tok, slot][:, None])
    return out


def _input(T, H, seed):
    # y = x . w has a standard deviation of about sqrt(H) * 0.9 * std(x) for random codes under scales 2^-5 .. 2^0: aim at ~3, so that the
    # clamps at +-7 are reached by a few percent of the values and most stay inside
    return (torch.randn(T, H, generator=torch.Generator().manual_seed(seed)) * (3.0 / (0.9 * H ** 0.5))).bfloat16()


# --- without a GPU ----------------------------------------------------------------------------------------------------------------

def _unpacked(ex):
    """GptOssExperts (CPU) -> per-expert dequantised f32 weights [E, 2 Ip, Hp] and [E, H, Ip], through the layout model's unpack and the oracle."""
    E, hp, ip, H = ex.num_experts, ex.hidden_padded, ex.inter_padded, ex.hidden
    q13 = LY.unpack_weights(ex.w13.numpy().view(np.uint32).ravel(), E * 2 * ip, hp).view(np.uint8).reshape(E * 2 * ip, hp // 2)
    s13 = LY.unpack_mxscales(ex.s13.numpy().ravel(), E * 2 * ip, hp).reshape(E * 2 * ip, hp // 32)
    q2 = LY.unpack_weights(ex.w2.numpy().view(np.uint32).ravel(), E * H, ip).view(np.uint8).reshape(E * H, ip // 2)
    s2 = LY.unpack_mxscales(ex.s2.numpy().ravel(), E * H, ip).reshape(E * H, ip // 32)
    return O.dequant_mxfp4(q13, s13).reshape(E, 2 * ip, hp), O.dequant_mxfp4(q2, s2).reshape(E, H, ip)


def _expected(ck, hp, ip, gate_parity=0):
    """The de-interleaved, zero-padded dequantisation of the checkpoint: f32 [E, 2 Ip, Hp] and [E, H, Ip]."""
    E, n13, hb, _ = ck["gate_up_blocks"].shape
    I, H = n13 // 2, hb * 32
    w13 = np.zeros((E, 2 * ip, hp), dtype=np.float32)
    w2 = np.zeros((E, H, ip), dtype=np.float32)
    for e in range(E):
        d = _dq(ck["gate_up_blocks"][e], ck["gate_up_scales"][e])
        w13[e, :I, :H] = d[gate_parity::2]
        w13[e, ip:ip + I, :H] = d[1 - gate_parity::2]
        w2[e, :, :I] = _dq(ck["down_blocks"][e], ck["down_scales"][e])
    return w13, w2


def test_prepare_equals_deinterleaved_padded_dequant_bit_for_bit():
    import petit_kernel as pk
    E, H, I = 4, 352, 352
    ck = synth_checkpoint(E, H, I, 1)
    ex = pk.prepare_gptoss_experts(**ck)
    assert (ex.hidden, ex.inter, ex.hidden_padded, ex.inter_padded, ex.num_experts) == (352, 352, 512, 512, 4)
    assert ex.w13.numel() * 4 == E * 1024 * 512 // 2 and ex.w2.numel() * 4 == E * 352 * 512 // 2
    assert torch.equal(ex.gs13, torch.ones(E)) and torch.equal(ex.gs2, torch.ones(E)) and ex.gs13.dtype == torch.float32
    got13, got2 = _unpacked(ex)
    want13, want2 = _expected(ck, 512, 512)
    assert np.array_equal(got13.view(np.uint32), want13.view(np.uint32)) and np.array_equal(got2.view(np.uint32), want2.view(np.uint32))
    # the padding really is zero rows / zero k-columns (code 0 under scale byte 127 = +0.0)
    assert not got13[:, I:512].any() and not got13[:, 512 + I:].any() and not got13[:, :, H:].any() and not got2[:, :, I:].any()
    # biases: de-interleaved, zero-padded, the caller's dtype
    b13 = ex.bias13.float().numpy()
    gb = ck["gate_up_bias"].float().numpy()
    assert ex.bias13.shape == (E, 1024) and ex.bias13.dtype == torch.bfloat16 and ex.bias2.shape == (E, H)
    assert np.array_equal(b13[:, :I], gb[:, 0::2]) and np.array_equal(b13[:, 512:512 + I], gb[:, 1::2])
    assert not b13[:, I:512].any() and not b13[:, 512 + I:].any()
    assert torch.equal(ex.bias2, ck["down_bias"])
    assert pk.prepare_gptoss_experts(**ck, dtype=torch.float16).bias13.dtype == torch.float16
    # the comparison can fail: the other nibble order, and the other gate / up parity
    swapped = dict(ck, gate_up_blocks=(ck["gate_up_blocks"] << 4) | (ck["gate_up_blocks"] >> 4), down_blocks=(ck["down_blocks"] << 4) | (ck["down_blocks"] >> 4))
    sw13, sw2 = _unpacked(pk.prepare_gptoss_experts(**swapped))
    assert not np.array_equal(sw13, want13) and not np.array_equal(sw2, want2)
    par13, _ = _expected(ck, 512, 512, gate_parity=1)
    assert not np.array_equal(got13, par13)
    # x padding
    x = torch.randn(3, H).bfloat16()
    xp = ex.pad_hidden(x)
    assert xp.shape == (3, 512) and torch.equal(xp[:, :H], x) and not xp[:, H:].any()


def test_shape_arithmetic_of_gpt_oss():
    from petit_kernel import gptoss
    assert gptoss.padded_size(2880) == 3072 and gptoss.padded_size(3072) == 3072 and gptoss.padded_size(352) == 512 and gptoss.padded_size(1) == 256
    E, H, I = 2, 2880, 2880
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    q13, sc13, b13, q2, sc2, b2 = gptoss.deinterleave_pad_gptoss(z(E, 2 * I, H // 32, 16), z(E, 2 * I, H // 32), torch.zeros(E, 2 * I).bfloat16(),
                                                                 z(E, H, I // 32, 16), z(E, H, I // 32), torch.zeros(E, H).bfloat16())
    assert q13.shape == (E, 6144, 1536) and sc13.shape == (E, 6144, 96) and b13.shape == (E, 6144)
    assert q2.shape == (E, 2880, 1536) and sc2.shape == (E, 2880, 96) and b2.shape == (E, 2880)
    assert (sc13[:, 2880:3072] == 127).all() and (sc13[:, :, 90:] == 127).all() and (sc2[:, :, 90:] == 127).all() and (sc13[:, :2880, :90] == 0).all()
    assert 6144 % 512 == 0 and 3072 % 256 == 0 and 2880 % 32 == 0      # the quantising epilogue's n, every kernel's k, down's n
    with pytest.raises(RuntimeError):
        gptoss.deinterleave_pad_gptoss(z(E, 2 * I + 1, H // 32, 16), z(E, 2 * I + 1, H // 32), torch.zeros(E, 2 * I + 1), z(E, H, I // 32, 16),
                                       z(E, H, I // 32), torch.zeros(E, H))


def test_layers_refuse_an_unknown_activation():
    import petit_kernel as pk
    x = torch.zeros(1, 256).bfloat16()
    for layer in (pk.fp4_moe, pk.fp4_moe_fused, pk.fp4_moe_native):
        with pytest.raises(RuntimeError, match="activation must be"):
            layer(x, x, x, torch.ones(2), x, x, torch.ones(2), torch.ones(1, 1), torch.zeros(1, 1, dtype=torch.int32), "mxfp4", activation="gelu")


# --- on the GPU -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pk():
    import petit_kernel
    assert torch.cuda.is_available()
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950")
    return petit_kernel


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _rel_rms(out, ref):
    err = out.float().cpu().numpy().astype(np.float64) - ref
    return np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2))


def _check_forward(pk, ck, ex, T, topk, seed):
    E, H = ex.num_experts, ex.hidden
    x = _input(T, H, seed)
    tw, ids = _routing(T, E, topk, seed)
    ref = gptoss_ref(ck, x, tw.numpy().astype(np.float64), ids.numpy())
    xd, twd, idd = x.to(DEV), tw.to(DEV), ids.to(DEV)
    fused = ex.forward(xd, twd, idd, path="fused")
    assert fused.shape == (T, H) and fused.dtype == torch.bfloat16
    r = _rel_rms(fused, ref)
    print(f"T {T} H {H}: fused vs f64 rel rms {r:.3e}")
    assert r <= 1e-2, r
    glue = pk.fp4_moe(ex.pad_hidden(xd), ex.w13, ex.s13, ex.gs13, ex.w2, ex.s2, ex.gs2, twd, idd, "mxfp4", bias13=ex.bias13, bias2=ex.bias2,
                      activation="swiglu_oai")
    assert np.abs(_u16(fused).astype(np.int32) - _u16(glue).astype(np.int32)).max() <= 1
    for fmt in ("mxfp8", "mxfp6", "mxfp4"):
        nat = ex.forward(xd, twd, idd, path="native", activations=fmt)
        assert nat.shape == (T, H) and nat.dtype == torch.bfloat16
        bound = 0.4 if fmt == "mxfp4" else 0.1
        rf = _rel_rms(nat, fused.float().cpu().numpy().astype(np.float64))
        rr = _rel_rms(nat, ref)
        print(f"T {T} H {H}: native {fmt} vs fused {rf:.3e}, vs f64 {rr:.3e}")
        assert rf < bound and rr < bound + 1e-2, (fmt, rf, rr)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5, 64])
def test_forward_small_vs_f64_reference(pk, T):
    """E = 8, top-4, H = I = 352 (pads to 512): both paths against the f64 gpt-oss block; fused agrees with the torch-glue layer within one ulp."""
    ck = synth_checkpoint(8, 352, 352, 20 + T)
    ex = pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in ck.items()})
    assert ex.w13.is_cuda and (ex.hidden_padded, ex.inter_padded) == (512, 512)
    # packed on the GPU = packed on the host and moved
    host = pk.prepare_gptoss_experts(**ck).to(DEV)
    for name in ("w13", "s13", "w2", "s2", "bias13", "bias2"):
        assert torch.equal(getattr(ex, name).view(torch.uint8), getattr(host, name).view(torch.uint8)), name
    _check_forward(pk, ck, ex, T, 4, T)


@pytest.fixture(scope="module")
def full_width(pk):
    ck = synth_checkpoint(32, 2880, 2880, 7)
    return ck, pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in ck.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 16])
def test_forward_full_width_vs_f64_reference(pk, full_width, T):
    """gpt-oss-20b's expert block: E = 32, top-4, H = I = 2880 -> 3072; the output is [T, 2880] with no slice."""
    ck, ex = full_width
    assert (ex.hidden, ex.inter, ex.hidden_padded, ex.inter_padded) == (2880, 2880, 3072, 3072)
    _check_forward(pk, ck, ex, T, 4, 100 + T)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "native"])
def test_unrouted_entries_contribute_nothing(pk, path):
    """-1 ids (experts that are not local under expert parallelism): the layer equals the f64 block that skips them, and, on the fused path,
    fp4_moe with those entries' router weights set to zero -- bias2 included, the weight multiplies down + bias."""
    E, topk, T = 8, 4, 40
    ck = synth_checkpoint(E, 352, 352, 3)
    ex = pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in ck.items()})
    x = _input(T, 352, 9)
    tw, ids = _routing(T, E, topk, 9)
    mask = torch.rand(T, topk, generator=torch.Generator().manual_seed(1)) < 0.3
    ids_m = torch.where(mask, -1, ids)
    out = ex.forward(x.to(DEV), tw.to(DEV), ids_m.to(DEV), path=path)
    ref = gptoss_ref(ck, x, tw.numpy().astype(np.float64), ids_m.numpy())
    assert _rel_rms(out, ref) <= (1e-2 if path == "fused" else 0.1 + 1e-2)
    if path == "fused":
        base = pk.fp4_moe(ex.pad_hidden(x.to(DEV)), ex.w13, ex.s13, ex.gs13, ex.w2, ex.s2, ex.gs2, torch.where(mask, 0.0, tw).to(DEV), ids.to(DEV),
                          "mxfp4", bias13=ex.bias13, bias2=ex.bias2, activation="swiglu_oai")
        assert np.abs(_u16(out).astype(np.int32) - _u16(base).astype(np.int32)).max() <= 1
    # a token whose every entry is unrouted gets exactly zero
    ids_z = ids_m.clone()
    ids_z[0] = -1
    assert not ex.forward(x.to(DEV), tw.to(DEV), ids_z.to(DEV), path=path)[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "native"])
def test_forward_graph_replay_with_a_second_routing(pk, path):
    """forward captured once under torch.cuda.graph (one capture stream, no parallel branches; the x padding is inside the capture) and
    replayed with other routings, one with -1 entries: each replay is bit-identical to the eager call."""
    E, topk, T, H = 8, 4, 16, 352
    ck = synth_checkpoint(E, H, H, 5)
    ex = pk.prepare_gptoss_experts(**{k: v.to(DEV) for k, v in ck.items()})
    tw0, id0 = _routing(T, E, topk, 0)
    sx, stw, stid = _input(T, H, 0).to(DEV), tw0.to(DEV), id0.to(DEV)

    def layer(xx, ww, ii):
        return ex.forward(xx, ww, ii, path=path)

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
    tw2, id2 = _routing(T, E, topk, 13)
    id2[::3, 1] = -1
    for i, (tw, tid) in enumerate([_routing(T, E, topk, 11), (tw2, id2)]):
        xi = _input(T, H, 50 + i).to(DEV)
        sx.copy_(xi)
        stw.copy_(tw.to(DEV))
        stid.copy_(tid.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        eager = layer(xi, tw.to(DEV), tid.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16)), f"replay {i} differs from the eager call"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nvfp4", "mxfp4"])
def test_layers_without_the_new_keywords_return_the_same_bits(pk, kind):
    """fp4_moe / fp4_moe_fused / fp4_moe_native called as before equal the calls with bias13=None, bias2=None, activation="silu_mul"."""
    from test_moe import _make_layer
    E, topk, hid, inter, T = 8, 2, 1024, 512, 48
    w13, w2 = _make_layer(pk, kind[:2], E, hid, inter, 41)
    x = torch.randn(T, hid, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16).to(DEV)
    tw, tid = _routing(T, E, topk, T)
    args = (x, w13.b, w13.sp, w13.gsd, w2.b, w2.sp, w2.gsd, tw.to(DEV), tid.to(DEV), kind)
    kw = dict(bias13=None, bias2=None, activation="silu_mul")
    for layer in (pk.fp4_moe, pk.fp4_moe_fused) + ((pk.fp4_moe_native,) if kind == "mxfp4" else ()):
        assert torch.equal(layer(*args).view(torch.int16), layer(*args, **kw).view(torch.int16)), layer.__name__
    # and the biases and the activation do reach the launches
    b13 = (torch.randn(E, 2 * inter, device=DEV) * 0.5).bfloat16()
    b2 = (torch.randn(E, hid, device=DEV) * 0.5).bfloat16()
    base = pk.fp4_moe_fused(*args)
    assert not torch.equal(base, pk.fp4_moe_fused(*args, bias13=b13)) and not torch.equal(base, pk.fp4_moe_fused(*args, bias2=b2))
    assert not torch.equal(base, pk.fp4_moe_fused(*args, activation="swiglu_oai"))

"""petit_kernel.gptoss -- the routed experts of a gpt-oss checkpoint (gpt-oss-20b / -120b: MXFP4 experts as shipped) on the MoE layers.

The checkpoint and the layers disagree in three places, and `prepare_gptoss_experts` settles all three once, at load time, with torch ops
only (CPU or GPU tensors):

  * gate and up rows are INTERLEAVED in `gate_up_proj` (gate = rows 0::2, up = rows 1::2, and the same for its bias); the fused epilogues
    want the [gate; up] halves of vLLM / SGLang's w13;
  * hidden = intermediate = 2880 is not a multiple of 256 (2880 % 256 = 64), the K granule of every kernel and the n % 512 of the
    quantising gate_up epilogue: both are zero-padded to 3072;
  * the activation is the clamped SwiGLU (activation="swiglu_oai"), and every expert has a bias on gate_up and on down.

The router's top-k (then softmax over the k) is `moe_route(..., scoring="softmax", renormalize=True)`: `GptOssExperts.forward_routed` starts
from the logits, `GptOssExperts.forward_hidden` one step earlier, from the hidden state and the router's weight and bias (the router's linear
runs as the library's router GEMM).  Attention sinks and the dense bf16 linears of gpt-oss are not this module's business.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

_PAD_TO = 256          # K granule of the kernels; 2 * (a multiple of 256) is the n % 512 of the quantising epilogue
_E8M0_ONE = 127        # the E8M0 byte of 2^0: the scale of a padded block (its codes are 0x0 = +0.0)


def padded_size(n: int) -> int:
    """n rounded up to the next multiple of 256 (2880 -> 3072)."""
    return (n + _PAD_TO - 1) // _PAD_TO * _PAD_TO


def _check(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(msg)


def deinterleave_pad_gptoss(gate_up_blocks, gate_up_scales, gate_up_bias, down_blocks, down_scales, down_bias):
    """The layout step alone, before any repacking: the checkpoint's tensors -> (q13, sc13, b13, q2, sc2, b2) with
    q13 uint8 [E, 2 Ip, Hp / 2] and sc13 uint8 [E, 2 Ip, Hp / 32] in [gate; up] order, b13 [E, 2 Ip], q2 uint8 [E, H, Ip / 2], sc2 uint8
    [E, H, Ip / 32], b2 [E, H]; two codes per byte, the lower-k element in the low nibble (the checkpoint's order and this library's)."""
    _check(gate_up_blocks.dtype == torch.uint8 and gate_up_blocks.dim() == 4 and gate_up_blocks.size(3) == 16,
           "gate_up_blocks must be uint8 [E, 2 I, H / 32, 16]")
    _check(down_blocks.dtype == torch.uint8 and down_blocks.dim() == 4 and down_blocks.size(3) == 16, "down_blocks must be uint8 [E, H, I / 32, 16]")
    E, n13, hb, _ = gate_up_blocks.shape
    _check(n13 % 2 == 0, "gate_up_blocks holds interleaved gate / up rows: an even number of them")
    inter, hidden = n13 // 2, hb * 32
    _check(tuple(down_blocks.shape) == (E, hidden, inter // 32, 16) and inter % 32 == 0,
           f"down_blocks must be [{E}, {hidden}, {inter} / 32, 16], got {tuple(down_blocks.shape)}")
    _check(hidden % 32 == 0, "the hidden size must be a multiple of 32 (down's N)")
    _check(gate_up_scales.dtype == torch.uint8 and tuple(gate_up_scales.shape) == (E, n13, hb), "gate_up_scales must be uint8 [E, 2 I, H / 32]")
    _check(down_scales.dtype == torch.uint8 and tuple(down_scales.shape) == (E, hidden, inter // 32), "down_scales must be uint8 [E, H, I / 32]")
    _check(tuple(gate_up_bias.shape) == (E, n13) and tuple(down_bias.shape) == (E, hidden), "biases must be [E, 2 I] and [E, H]")
    ip, hp = padded_size(inter), padded_size(hidden)
    dev = gate_up_blocks.device

    q_in = gate_up_blocks.reshape(E, n13, hidden // 2)
    q13 = torch.zeros((E, 2 * ip, hp // 2), dtype=torch.uint8, device=dev)
    sc13 = torch.full((E, 2 * ip, hp // 32), _E8M0_ONE, dtype=torch.uint8, device=dev)
    b13 = torch.zeros((E, 2 * ip), dtype=gate_up_bias.dtype, device=dev)
    for half, row0 in ((0, 0), (1, ip)):          # gate = rows 0::2 -> [0, I); up = rows 1::2 -> [Ip, Ip + I)
        q13[:, row0:row0 + inter, :hidden // 2] = q_in[:, half::2]
        sc13[:, row0:row0 + inter, :hb] = gate_up_scales[:, half::2]
        b13[:, row0:row0 + inter] = gate_up_bias[:, half::2]

    q2 = torch.zeros((E, hidden, ip // 2), dtype=torch.uint8, device=dev)
    sc2 = torch.full((E, hidden, ip // 32), _E8M0_ONE, dtype=torch.uint8, device=dev)
    q2[:, :, :inter // 2] = down_blocks.reshape(E, hidden, inter // 2)
    sc2[:, :, :inter // 32] = down_scales
    return q13, sc13, b13, q2, sc2, down_bias.contiguous()


@dataclass
class GptOssExperts:
    """What prepare_gptoss_experts returns: the arguments of fp4_moe / fp4_moe_fused / fp4_moe_native (kind='mxfp4') for one MoE block."""
    w13: torch.Tensor      # repack_mxfp4 of the stacked [E * 2 Ip, Hp] gate_up weights, [gate; up] per expert
    s13: torch.Tensor      # process_mxfp4_scales of their [E * 2 Ip, Hp / 32] scales
    w2: torch.Tensor       # the same for the stacked [E * H, Ip] down weights
    s2: torch.Tensor
    gs13: torch.Tensor     # ones [E]: MXFP4 has no global scale
    gs2: torch.Tensor
    bias13: torch.Tensor   # [E, 2 Ip], [gate; up], zero in the padding
    bias2: torch.Tensor    # [E, H]
    hidden: int
    inter: int
    hidden_padded: int
    inter_padded: int

    @property
    def num_experts(self) -> int:
        return self.gs13.numel()

    def to(self, device) -> "GptOssExperts":
        """The same block with every tensor on `device` (a block prepared from CPU tensors is moved once, after loading)."""
        moved = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        return GptOssExperts(**moved)

    def pad_hidden(self, x: torch.Tensor) -> torch.Tensor:
        """x [T, hidden] -> [T, hidden_padded] with zero columns (one torch op; x itself when no padding is needed)."""
        _check(x.dim() == 2 and x.size(1) == self.hidden, f"x must be [T, {self.hidden}]")
        return x if self.hidden_padded == self.hidden else torch.nn.functional.pad(x, (0, self.hidden_padded - self.hidden))

    def forward(self, x: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, path: str = "fused",
                activations: str = "mxfp8", invariant: bool = False) -> torch.Tensor:
        """The expert block of gpt-oss: out[t] = sum_j topk_weights[t, j] * (down_e(swiglu_oai(gate_up_e(x_t) + b13_e)) + b2_e), e = topk_ids[t, j].

        x [T, hidden] bf16 / fp16 (the biases' dtype); returns [T, hidden] -- down's N is the unpadded hidden size, so nothing is sliced off.
        path 'fused': fp4_moe_fused (exact class); 'native': fp4_moe_native with `activations` ('mxfp8' / 'mxfp6' / 'mxfp4').
        Cost of the padding: x is zero-padded to hidden_padded with one torch op, i.e. one T x hidden_padded 16-bit copy per call (18 KiB per
        token at 2880 -> 3072: the kernels read A in whole 256-column spans and have no column mask).  No host sync: capturable.
        invariant=True: the layer's batch-invariant switch on either path (fp4_moe_fused / fp4_moe_native, invariant=True): a token's output
        row has the same bits alone and inside any batch.  Path 'native' takes bf16 and fp16; path 'fused' bf16 only."""
        from .moe import fp4_moe_fused, fp4_moe_native
        _check(path in ("fused", "native"), "path must be 'fused' or 'native'")
        xp = self.pad_hidden(x)
        kw = dict(bias13=self.bias13, bias2=self.bias2, activation="swiglu_oai")
        if path == "fused":
            return fp4_moe_fused(xp, self.w13, self.s13, self.gs13, self.w2, self.s2, self.gs2, topk_weights, topk_ids, kind="mxfp4",
                                 invariant=invariant, **kw)
        return fp4_moe_native(xp, self.w13, self.s13, self.gs13, self.w2, self.s2, self.gs2, topk_weights, topk_ids, kind="mxfp4",
                              activations=activations, invariant=invariant, **kw)

    def forward_routed(self, x: torch.Tensor, router_logits: torch.Tensor, topk: int = 4, path: str = "fused",
                       activations: str = "mxfp8") -> torch.Tensor:
        """forward from the router's logits [T, E] (float32 / bfloat16 / float16): gpt-oss's routing -- the top-k logits, softmax over the k --
        by moe_route_align, then forward's launches: bit for bit forward(x, *moe_route(router_logits, topk), path, activations)."""
        from .moe import fp4_moe_routed
        _check(path in ("fused", "native"), "path must be 'fused' or 'native'")
        return fp4_moe_routed(self.pad_hidden(x), router_logits, self.w13, self.s13, self.gs13, self.w2, self.s2, self.gs2, topk, kind="mxfp4",
                              path=path, activations=activations, bias13=self.bias13, bias2=self.bias2, activation="swiglu_oai",
                              scoring="softmax", renormalize=True)

    def forward_hidden(self, x: torch.Tensor, router_weight: torch.Tensor, router_bias: torch.Tensor = None, topk: int = 4, path: str = "fused",
                       activations: str = "mxfp8") -> torch.Tensor:
        """forward from the hidden state: the router's linear x . router_weight [E, hidden]^T + router_bias (float32 [E]) as the library's
        router GEMM on the UNPADDED x (K = 2880), the routing on its partial sums, then forward's launches on pad_hidden(x): bit for bit
        forward_routed(x, moe_router_logits(x, router_weight, router_bias), topk, path, activations)."""
        from .moe import fp4_moe_routed
        _check(path in ("fused", "native"), "path must be 'fused' or 'native'")
        return fp4_moe_routed(self.pad_hidden(x), None, self.w13, self.s13, self.gs13, self.w2, self.s2, self.gs2, topk, kind="mxfp4",
                              path=path, activations=activations, bias13=self.bias13, bias2=self.bias2, activation="swiglu_oai",
                              router_weight=router_weight, router_bias=router_bias, router_input=x, scoring="softmax", renormalize=True)


def prepare_gptoss_experts(gate_up_blocks: torch.Tensor, gate_up_scales: torch.Tensor, gate_up_bias: torch.Tensor, down_blocks: torch.Tensor,
                           down_scales: torch.Tensor, down_bias: torch.Tensor, dtype: torch.dtype = None) -> GptOssExperts:
    """The expert tensors of one gpt-oss MoE block, as the checkpoint stores them, -> GptOssExperts.

    gate_up_blocks uint8 [E, 2 I, H / 32, 16], gate_up_scales E8M0 uint8 [E, 2 I, H / 32], gate_up_bias [E, 2 I]: rows (and bias entries)
    interleaved, gate = 0::2, up = 1::2.  down_blocks uint8 [E, H, I / 32, 16], down_scales uint8 [E, H, I / 32], down_bias [E, H].  Blocks
    hold two E2M1 codes per byte, the lower-k element in the low nibble.  dtype: the biases' (= the activations') dtype, default
    gate_up_bias's.  All tensors on one device; CPU tensors are packed by the library's host path, GPU tensors by its kernels.

    Steps: de-interleave the rows to [gate; up]; zero-pad I to the next multiple of 256 -- as rows in EACH half of gate_up, as k-columns
    in down -- and H (gate_up's K) as k-columns; zero-pad the biases; repack_mxfp4 / process_mxfp4_scales of the stacked tensors.  A zero
    column is code 0x0 (+0.0) under scale byte 127 (2^0).  Down's N stays H, so the layer's output is [T, H] with no slice.

    Why the padding changes nothing: x's padded columns are zeros against zero weights, exact zeros in every accumulation.  A padded
    gate / up column j has zero weights and a zero bias, so y_gate = y_up = 0, g = min(0, 7) = 0 and the activation is
    0 * sigmoid(0) * (0 + 1) = exactly 0 (SiLU-mul gives 0 * 0 too); down multiplies that 0 by its zero k-columns.  On the native path the
    zeros of a partly padded 32-block do not move the block maximum, and a wholly padded block quantises to codes 0 under scale 2^0."""
    q13, sc13, b13, q2, sc2, b2 = deinterleave_pad_gptoss(gate_up_blocks, gate_up_scales, gate_up_bias, down_blocks, down_scales, down_bias)
    E, n13p, hp2 = q13.shape
    hidden, ip = q2.size(1), q2.size(2) * 2
    hp, inter = hp2 * 2, gate_up_blocks.size(1) // 2
    if q13.is_cuda:
        from . import process_mxfp4_scales as scales_fn, repack_mxfp4 as repack_fn
    else:
        from .offline import process_mxfp4_scales_cpu as scales_fn, repack_mxfp4_cpu as repack_fn
    w13 = repack_fn(q13.reshape(E * n13p, hp // 2).view(torch.int32), E * n13p, hp)
    s13 = scales_fn(sc13.reshape(E * n13p, hp // 32), E * n13p, hp)
    w2 = repack_fn(q2.reshape(E * hidden, ip // 2).view(torch.int32), E * hidden, ip)
    s2 = scales_fn(sc2.reshape(E * hidden, ip // 32), E * hidden, ip)
    dtype = dtype or gate_up_bias.dtype
    _check(dtype in (torch.bfloat16, torch.float16), "the biases (and activations) must be bfloat16 or float16")
    ones = torch.ones(E, dtype=torch.float32, device=q13.device)
    return GptOssExperts(w13=w13, s13=s13, w2=w2, s2=s2, gs13=ones, gs2=ones.clone(), bias13=b13.to(dtype).contiguous(),
                         bias2=b2.to(dtype).contiguous(), hidden=hidden, inter=inter, hidden_padded=hp, inter_padded=ip)

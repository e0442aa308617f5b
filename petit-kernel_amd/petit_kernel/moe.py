"""petit_kernel.moe -- a routed-expert (mixture-of-experts) FP4 layer on the MoE launch (include/petit_amd.h "Routed-expert (MoE) launch").

`moe_align` sorts the (token, slot) pairs of a top-k routing by expert and counts them per expert -- torch ops only, no host sync, so the
whole layer can be captured in a graph and replayed with a different routing.  `fp4_moe` runs gate_up (fused SiLU-mul) and down as one
MoE launch each; the router weighting and the top-k combine are torch plumbing, in fp32, in a fixed order (deterministic).

`fp4_moe_fused` is the same layer in four launches of the library's own (one to three for the align, then gate_up, down, combine): the
align runs on the device, gate_up reads the token rows through the sorted index (no gathered copy of the activations), down writes each
(token, slot) result straight to its slot, and a deterministic top-k reduce finishes the layer.  Ids of -1 (experts that are not local
under expert parallelism) are skipped.

`fp4_moe_routed` starts one step earlier, from the router's logits: `moe_route_align` (top-k ids and weights with a stated tie rule, fused
with the align into one launch for every decode batch), then the launches of `fp4_moe_fused` or `fp4_moe_native`.
"""
from __future__ import annotations

import torch


def moe_align(topk_ids: torch.Tensor, num_experts: int):
    """topk_ids [T, topk] (any integer dtype) -> (sorted_idx, expert_offsets).

    sorted_idx: int64 [T * topk], the flattened (token, slot) positions grouped by expert (stable: ascending position inside an expert);
    position p is token p // topk.  expert_offsets: int32 [num_experts + 1], rows expert_offsets[e] .. expert_offsets[e+1]-1 of the grouped
    order belong to expert e.  Works on CPU and GPU tensors alike and never synchronises with the device."""
    flat = topk_ids.reshape(-1).to(torch.int64)
    sorted_idx = torch.argsort(flat, stable=True)
    counts = torch.zeros(num_experts, dtype=torch.int32, device=flat.device)
    counts.scatter_add_(0, flat, torch.ones_like(flat, dtype=torch.int32))
    offsets = torch.zeros(num_experts + 1, dtype=torch.int32, device=flat.device)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int32)
    return sorted_idx, offsets


def _check_activation(activation) -> None:
    if activation not in ("silu_mul", "swiglu_oai"):
        raise RuntimeError("activation must be 'silu_mul' or 'swiglu_oai'")


def _down_n(w2: torch.Tensor, num_experts: int, inter: int, hidden: int) -> int:
    """N of the down launch: the rows of one expert's packed [N, I] FP4 weight (half a byte per element).  It equals hidden's width unless the
    caller padded hidden's K for gate_up alone (petit_kernel.gptoss: 2880 -> 3072 columns in, 2880 out)."""
    n2 = w2.numel() * w2.element_size() * 2 // (num_experts * inter)
    if n2 > hidden:
        raise RuntimeError(f"w2 holds [{n2}, {inter}] per expert, more rows than hidden's width {hidden}")
    return n2


def fp4_moe(hidden: torch.Tensor, w13: torch.Tensor, s13: torch.Tensor, gs13: torch.Tensor, w2: torch.Tensor, s2: torch.Tensor,
            gs2: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, kind: str = "nvfp4", *, bias13: torch.Tensor = None,
            bias2: torch.Tensor = None, activation: str = "silu_mul") -> torch.Tensor:
    """A gated-MLP MoE layer: out[t] = sum_j topk_weights[t, j] * down_e(silu(gate_e(x_t)) * up_e(x_t)), e = topk_ids[t, j].

    hidden [T, H] bf16 / fp16.  w13 / s13: the E experts' [gate; up] weights ([2 I, H] each, vLLM / SGLang's w13 layout) packed back to
    back -- repack_* / process_*_scales of the stacked [E * 2 I, H] tensors; w2 / s2 the same for the [H, I] down weights; gs13 / gs2:
    float32 [E] global scales.  kind: 'nvfp4' or 'mxfp4'.  Returns [T, H] in hidden's dtype.

    bias13 [E, 2 I] (in [gate; up] order) and bias2 [E, H], in hidden's dtype, are added by the gate_up and the down launch: the router
    weight multiplies down + bias2.  activation: 'silu_mul', or 'swiglu_oai' (gpt-oss: min(gate, 7) * sigmoid(1.702 gate) * (clamp(up, -7, 7)
    + 1) on gate_up + bias13).  down's K is I and its N the hidden size of `w2`, which may be smaller than hidden's (petit_kernel.gptoss
    pads K only).  With the defaults the layer issues the launches it always issued."""
    from . import mul_mxfp4_a16_moe, mul_nvfp4_a16_moe
    if kind not in ("nvfp4", "mxfp4"):
        raise RuntimeError("kind must be 'nvfp4' or 'mxfp4'")
    _check_activation(activation)
    mul = mul_nvfp4_a16_moe if kind == "nvfp4" else mul_mxfp4_a16_moe
    T, H = hidden.shape
    topk = topk_ids.shape[1]
    E = gs13.numel()
    n13 = w13.numel() * w13.element_size() * 2 // (E * H)   # 2 I
    inter = n13 // 2
    m = T * topk
    sorted_idx, offsets = moe_align(topk_ids, E)
    a = hidden.index_select(0, sorted_idx // topk)                                        # rows grouped by expert
    n2 = _down_n(w2, E, inter, H)
    h = mul(a, w13, s13, gs13, offsets, m, n13, H, E, bias=bias13, activation=activation)  # [m, I]
    y = mul(h, w2, s2, gs2, offsets, m, n2, inter, E, bias=bias2)                          # [m, n2]
    w = topk_weights.reshape(-1).to(torch.float32).index_select(0, sorted_idx)
    buf = torch.empty((m, n2), dtype=torch.float32, device=hidden.device)
    buf.index_copy_(0, sorted_idx, y.float() * w[:, None])                                # every (token, slot) position exactly once
    return buf.view(T, topk, n2).sum(dim=1).to(hidden.dtype)


def fp4_moe_fused(hidden: torch.Tensor, w13: torch.Tensor, s13: torch.Tensor, gs13: torch.Tensor, w2: torch.Tensor, s2: torch.Tensor,
                  gs2: torch.Tensor, topk_weights: torch.Tensor, topk_ids: torch.Tensor, kind: str = "nvfp4", *, bias13: torch.Tensor = None,
                  bias2: torch.Tensor = None, activation: str = "silu_mul", norm_weight: torch.Tensor = None, norm_eps: float = 1e-6,
                  norm_residual: torch.Tensor = None, norm_weight_offset: float = 0.0, norm_fmt: str = None, invariant: bool = False):
    """fp4_moe's layer (same arguments, same result up to the combine's rounding order) on the indexed MoE launches: align on the device,
    gate_up on gathered rows, down scattered into slot order, the top-k combine.  topk_ids: int32 or int64 [T, topk]; entries outside
    [0, E) (-1 under expert parallelism) contribute nothing.  topk_weights: float32 or bfloat16 [T, topk] (converted to float32 once).
    bias13 / bias2 / activation: as fp4_moe (the biases ride in the gate_up and down launches: no launch more).
    No host sync: capturable in a graph and replayable with any routing of the same shape.

    norm_weight (with norm_eps, norm_residual, norm_weight_offset, norm_fmt): the fused end -- the layer ends in moe_combine_rmsnorm instead of
    moe_combine, one launch for the combine, the residual add (norm_residual), the next block's RMSNorm (norm_weight [H]) and, with norm_fmt
    ('mxfp8' / 'mxfp6' / 'mxfp4'), its activation quantiser.  Returns (h, y16) with norm_fmt None and (q, h) with one: h = layer output (+
    norm_residual) in 16 bits, y16 = RMSNorm(h) * (norm_weight + norm_weight_offset), q = quantize_activations(y16, norm_fmt), each bit for bit
    what the un-fused layer followed by rmsnorm_quantize gives.  The fused end is for a layer whose combine is COMPLETE on this rank: under
    tensor or expert parallelism an all-reduce belongs between the combine and the residual add, so such a layer ends in moe_combine.
    Measured (profiles/moe_combine_norm.md) against moe_combine followed by the norm.

    invariant=True: gate_up and down run as the batch-invariant MoE launches (mul_*_a16_moe_invariant) in place of the indexed ones;
    everything else is unchanged.  Every slot row is then a pure function of its token's hidden row and its expert's weights, and the
    combine adds a token's slots in slot order, in fp32, with one rounding: given the same topk_weights / topk_ids row, a token's output row
    has the same bits alone and inside any batch, at any position.  This holds with the fused norm end too (both returned tensors: the norm
    works per row).  Under expert or tensor parallelism it holds only up to the all-reduce, which is outside this library.  Opt-in and slower
    (profiles/moe_invariant.md); float16 hidden states with kind 'mxfp4' have no batch-invariant kernel."""
    _check_fused(kind, activation)
    _check_invariant_layer(invariant, "fused", kind, hidden)
    norm = _norm_end(norm_weight, norm_eps, norm_residual, norm_weight_offset, norm_fmt)
    w, ids, sorted_pos, offsets, token_index = _align_routing(topk_weights, topk_ids, gs13.numel())
    return _fused_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, kind, bias13, bias2, activation, norm,
                              invariant)


def _norm_end(norm_weight, norm_eps, norm_residual, norm_weight_offset, norm_fmt):
    """The fused end of a layer as its last step takes it: None (the layer ends in moe_combine) or moe_combine_rmsnorm's arguments."""
    if norm_weight is None:
        if norm_residual is not None or norm_fmt is not None:
            raise RuntimeError("norm_residual / norm_fmt need a norm_weight (the fused end of the layer)")
        return None
    return dict(weight=norm_weight, eps=norm_eps, fmt=norm_fmt, residual=norm_residual, weight_offset=norm_weight_offset, return_hidden=True)


def _combine(y, w, ids, num_experts, norm):
    """The last launch of a layer: the top-k combine, or with a fused end the combine into the norm."""
    from . import moe_combine, moe_combine_rmsnorm
    return moe_combine(y, w, ids, num_experts) if norm is None else moe_combine_rmsnorm(y, w, ids, num_experts, **norm)


def _align_routing(topk_weights, topk_ids, num_experts):
    """The routing as the fused and native layers take it: (float32 weights, int32 / int64 ids, both contiguous, then moe_align_device of the ids)."""
    from . import moe_align_device
    ids = topk_ids if topk_ids.dtype in (torch.int32, torch.int64) and topk_ids.is_contiguous() else topk_ids.contiguous().to(torch.int64)
    w = topk_weights if topk_weights.dtype == torch.float32 and topk_weights.is_contiguous() else topk_weights.float().contiguous()
    return (w, ids) + tuple(moe_align_device(ids, num_experts))


def _check_fused(kind, activation) -> None:
    if kind not in ("nvfp4", "mxfp4"):
        raise RuntimeError("kind must be 'nvfp4' or 'mxfp4'")
    _check_activation(activation)


def _check_invariant_layer(invariant, path, kind, hidden) -> None:
    if not invariant:
        return
    if path == "native":
        raise RuntimeError("invariant=True is for path 'fused': the native class quantises activations per call and has no batch-invariant "
                           "kernel")
    if kind == "mxfp4" and hidden.dtype == torch.float16:
        raise RuntimeError("invariant=True with kind 'mxfp4' needs bfloat16 hidden states: float16 activations with MXFP4 weights have no "
                           "batch-invariant kernel")


def _fused_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, kind, bias13, bias2, activation, norm=None,
                       invariant=False):
    """fp4_moe_fused after its align: gate_up on gathered rows, down scattered into slot order, the combine (w float32, ids int32 / int64).
    invariant: the two launches are the batch-invariant ones."""
    from . import mul_mxfp4_a16_moe_indexed, mul_mxfp4_a16_moe_invariant, mul_nvfp4_a16_moe_indexed, mul_nvfp4_a16_moe_invariant
    if invariant:
        mul = mul_nvfp4_a16_moe_invariant if kind == "nvfp4" else mul_mxfp4_a16_moe_invariant
    else:
        mul = mul_nvfp4_a16_moe_indexed if kind == "nvfp4" else mul_mxfp4_a16_moe_indexed
    T, H = hidden.shape
    topk = ids.shape[1]
    E = gs13.numel()
    n13 = w13.numel() * w13.element_size() * 2 // (E * H)   # 2 I
    inter = n13 // 2
    m = T * topk
    n2 = _down_n(w2, E, inter, H)
    h = mul(hidden, w13, s13, gs13, offsets, m, n13, H, E, a_row_index=token_index, bias=bias13, activation=activation)  # [m, I], grouped order
    y = mul(h, w2, s2, gs2, offsets, m, n2, inter, E, c_row_index=sorted_pos, c_rows=m, bias=bias2)          # [m, n2], (token, slot) order
    return _combine(y, w, ids, E, norm)


_NATIVE_SENTINELS = {"mxfp8": -2, "mxfp4": -3, "mxfp6": -4}   # SOLUTION_AUTO_NATIVE_MXFP8 / _MXFP4 / _MXFP6


def fp4_moe_native(hidden: torch.Tensor, w13: torch.Tensor, s13, gs13: torch.Tensor, w2: torch.Tensor, s2, gs2: torch.Tensor,
                   topk_weights: torch.Tensor, topk_ids: torch.Tensor, kind: str = "mxfp4", activations: str = "mxfp8", *,
                   bias13: torch.Tensor = None, bias2: torch.Tensor = None, activation: str = "silu_mul", transient: bool = False,
                   norm_weight: torch.Tensor = None, norm_eps: float = 1e-6, norm_residual: torch.Tensor = None, norm_weight_offset: float = 0.0,
                   norm_fmt: str = None, invariant: bool = False):
    """fp4_moe_fused's layer on the NATIVE class (the block-scaled MFMA, activations quantised to `activations`: 'mxfp8', 'mxfp6' or 'mxfp4';
    petit_gemm_native_moe -- a different accuracy class than the exact layers).  kind 'mxfp4': w13 / s13 / w2 / s2 as fp4_moe_fused; kind
    'nvfp4': w13 / w2 are the experts' MFMA-native images back to back (nvfp4_native_images) and s13 / s2 are None.  Five launches (seven
    when the align needs its three-launch form): the device align, the gathering quantiser, gate_up with SiLU-mul writing the quantised
    grouped rows down reads, down scattered into slot order, the top-k combine.  bias13 / bias2 / activation: as fp4_moe; 'swiglu_oai' is
    quantised for down from its f32 value, as SiLU-mul is.  No host sync: capturable.

    transient=True (kind 'nvfp4' only): w13 / s13 / w2 / s2 are the PACKED stacked tensors, as fp4_moe_fused takes them, and no image stays
    resident: each of the two launches is mul_nvfp4_native_moe_transient, which first builds the images of the experts this routing uses
    into the scratch (one more launch each).  Both launches run one after the other on ONE scratch buffer, which the layer takes from the
    allocator for the call (the larger of the two launches' workspace queries) and releases on return: the layer holds 4.5 bits per weight
    and, while it runs, that scratch.  Bit for bit the resident layer on nvfp4_native_images of the same tensors.

    norm_weight / norm_eps / norm_residual / norm_weight_offset / norm_fmt: fp4_moe_fused's fused end (the combine, the residual add, the next
    RMSNorm and its quantiser in the last launch; returns (h, y16) or (q, h)), for a layer whose combine is complete on this rank.

    invariant=True (kind 'mxfp4', resident tensors): gate_up and down run as the native class's batch-invariant MoE launches
    (mul_mxfp4_native_moe_invariant): the device align, the gathering quantiser, gate_up on the quantised grouped rows with the gated
    activation writing 16-bit [m, I] grouped rows, down on that matrix -- which quantises it itself -- scattered into slot order, the combine.
    Every slot row is then a pure function of its token's hidden row and its expert's weights, and the combine adds a token's slots in slot
    order, in fp32, with one rounding: given the same topk_weights / topk_ids row, a token's output row has the same bits alone and inside
    any batch, at any position -- with the fused norm end too.  bfloat16 and float16 hidden states.  Opt-in and slower
    (profiles/native_moe_invariant.md).  kind 'nvfp4' and transient=True raise: images are not on the invariant native entries."""
    _check_native(kind, activation, activations, transient)
    if invariant:
        if transient:
            raise RuntimeError("invariant=True on the native class does not take transient=True: images have no batch-invariant native kernel")
        if kind == "nvfp4":
            raise RuntimeError("invariant=True on the native class is for kind 'mxfp4': NVFP4 images have no batch-invariant native kernel "
                               "(fp4_moe_fused(..., invariant=True) runs NVFP4 experts in the exact class)")
    norm = _norm_end(norm_weight, norm_eps, norm_residual, norm_weight_offset, norm_fmt)
    w, ids, sorted_pos, offsets, token_index = _align_routing(topk_weights, topk_ids, gs13.numel())
    if invariant:
        return _native_invariant_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, activations, bias13,
                                             bias2, activation, norm)
    return _native_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, kind, activations, bias13, bias2,
                               activation, transient, norm)


def _check_native(kind, activation, activations, transient=False) -> None:
    if kind not in ("nvfp4", "mxfp4"):
        raise RuntimeError("kind must be 'nvfp4' or 'mxfp4'")
    _check_activation(activation)
    if activations not in _NATIVE_SENTINELS:
        raise RuntimeError("activations must be 'mxfp8', 'mxfp6' or 'mxfp4'")
    if transient and kind != "nvfp4":
        raise RuntimeError("transient=True is for kind 'nvfp4' (MXFP4 experts run on the packed tensors: there is no image to build)")


def _native_invariant_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, activations, bias13, bias2,
                                  activation, norm=None):
    """fp4_moe_native(invariant=True) after its align: the gathering quantiser, the two batch-invariant launches, the combine."""
    from . import mul_mxfp4_native_moe_invariant, quantize_activation_rows
    T, H = hidden.shape
    E = gs13.numel()
    m = T * ids.shape[1]
    n13 = w13.numel() * w13.element_size() * 2 // (E * H)   # 2 I
    inter = n13 // 2
    n2 = _down_n(w2, E, inter, H)
    qa = quantize_activation_rows(hidden, activations, token_index)                  # grouped rows; unrouted (-1) rows are zeros
    h = mul_mxfp4_native_moe_invariant(qa, w13, s13, gs13, offsets, m, n13, H, E, fmt=activations, bias=bias13, activation=activation)  # [m, I]
    y = mul_mxfp4_native_moe_invariant(h, w2, s2, gs2, offsets, m, n2, inter, E, c_row_index=sorted_pos, c_rows=m, fmt=activations,
                                       bias=bias2)                                   # [m, n2], (token, slot) order
    return _combine(y, w, ids, E, norm)


def _native_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, kind, activations, bias13, bias2,
                        activation, transient=False, norm=None):
    """fp4_moe_native after its align: the gathering quantiser, gate_up, down scattered into slot order, the combine."""
    from . import mul_mxfp4_native_moe, mul_nvfp4_native_moe, mul_nvfp4_native_moe_transient, quantize_activation_rows
    sid = _NATIVE_SENTINELS[activations]
    T, H = hidden.shape
    E = gs13.numel()
    m = T * ids.shape[1]
    if kind == "mxfp4" or transient:                            # packed stacked tensors
        n13 = w13.numel() * w13.element_size() * 2 // (E * H)   # 2 I
        inter = n13 // 2
        n2 = _down_n(w2, E, inter, H)
        mul, gate_up, down = (mul_nvfp4_native_moe_transient if transient else mul_mxfp4_native_moe), (w13, s13, gs13), (w2, s2, gs2)
    else:
        n13 = w13.numel() * 32 // (E * H * 25)                  # an image holds 25 / 32 bytes per weight (6.25 bits)
        inter = n13 // 2
        n2 = H
        mul, gate_up, down = mul_nvfp4_native_moe, (w13, gs13), (w2, gs2)
    qa = quantize_activation_rows(hidden, activations, token_index)                  # grouped rows; unrouted (-1) rows are zeros
    ws = {}
    if transient:   # one scratch for both launches (a_format: both take quantised rows where gate_up hands them over; else down quantises)
        from . import nvfp4_native_moe_transient_workspace_bytes as query
        quantised = n13 % 512 == 0
        need = max(query(E, m, n13, H, sid, hidden.dtype, activation, activations, activations if quantised else None),
                   query(E, m, n2, inter, sid, hidden.dtype, None, activations if quantised else None, None))
        if need:    # (0: nothing to do, or a call the launch itself refuses with its own message)
            ws = {"workspace": torch.empty(need, dtype=torch.uint8, device=hidden.device)}
    # gate_up writes down's quantised input, grouped, where its tiles allow; else 16-bit, and down quantises it (one more launch)
    h = mul(qa, *gate_up, offsets, m, n13, H, E, solution_id=sid, bias=bias13, activation=activation,
            out_quantized=activations if n13 % 512 == 0 else None, **ws)
    y = mul(h, *down, offsets, m, n2, inter, E, solution_id=sid, c_row_index=sorted_pos, c_rows=m, bias=bias2, **ws)   # [m, n2], (token, slot) order
    return _combine(y, w, ids, E, norm)


def fp4_moe_routed(hidden: torch.Tensor, router_logits: torch.Tensor, w13: torch.Tensor, s13, gs13: torch.Tensor, w2: torch.Tensor, s2,
                   gs2: torch.Tensor, topk: int, kind: str = "nvfp4", *, path: str = "fused", activations: str = "mxfp8",
                   bias13: torch.Tensor = None, bias2: torch.Tensor = None, activation: str = "silu_mul", transient: bool = False,
                   norm_weight: torch.Tensor = None, norm_eps: float = 1e-6, norm_residual: torch.Tensor = None, norm_weight_offset: float = 0.0,
                   norm_fmt: str = None, router_weight: torch.Tensor = None, router_bias: torch.Tensor = None,
                   router_input: torch.Tensor = None, invariant: bool = False, **routing):
    """The layer from the router's logits: moe_route_align(router_logits, topk, **routing), then exactly the launches fp4_moe_fused (path
    'fused') or fp4_moe_native (path 'native', with `activations`) issue after their align -- bit for bit
    fp4_moe_fused(..., *moe_route(router_logits, topk, **routing)).  router_logits [T, E] float32 / bfloat16 / float16; routing: moe_route's
    keyword arguments (scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor).  Route and align are ONE launch when
    T * topk <= 1024 (the fused layer: 4 launches; 7 above).  No host sync: capturable, and a routing is a pure function of the logits.

    routing also takes moe_route's slot-list arguments (expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits): the
    same launches on topk + num_shared slots per token.  router_logits is always [T, number of GLOBAL experts]; the weight stacks (w13 / s13 /
    gs13 / w2 / s2 / gs2, bias13 / bias2) hold the LOCAL routed experts followed by the shared ones: router_logits.size(1) + num_shared
    experts without an expert_map, num_local_experts + num_shared with one.  A shared expert is of the routed experts' size (a k times wider
    one is k shared experts).  One launch for route + align when T * (topk + num_shared) <= 1024.

    transient (path 'native', kind 'nvfp4'): fp4_moe_native's switch -- the packed tensors, no resident images.

    router_weight (with router_logits None; router_bias float32 [E] optional): the layer from the hidden state.  The router's linear
    hidden . router_weight[E, K]^T (+ router_bias) runs as the library's router GEMM and moe_route_hidden takes moe_route_align's place: one
    launch more than from the logits (5 for the fused layer at T * topk <= 1024), bit for bit
    fp4_moe_routed(hidden, moe_router_logits(hidden, router_weight, router_bias), ...).  The router reads `hidden`, or router_input [T, k] when the
    experts' `hidden` is a padded copy of it (gpt-oss: 2880 columns against 3072).

    norm_weight / norm_eps / norm_residual / norm_weight_offset / norm_fmt: fp4_moe_fused's fused end on either path (returns (h, y16) or
    (q, h)): with route + align in one launch the whole layer and the next block's norm are four launches.  For a layer whose combine is complete
    on this rank (no all-reduce between the combine and the residual add).

    invariant=True (path 'fused'): fp4_moe_fused's switch -- gate_up and down run as the batch-invariant MoE launches.  From
    router_weight=... (or from router_logits that are themselves batch-invariant) the whole layer is then batch-invariant: the router's
    logits, with the tie rule the chosen experts and their weights, every slot row and the combine are pure functions of the token's hidden
    row and the weights, so a token's output row has the same bits alone and inside any batch.  This holds with the fused norm end too (both
    returned tensors).  Under expert or tensor parallelism it holds only up to the all-reduce, which is outside this library.  path 'native'
    and kind 'mxfp4' on float16 hidden states raise here: the native class's batch-invariant layer is fp4_moe_native(..., invariant=True), from
    a routing computed by the caller (moe_route_hidden)."""
    from . import moe_route_align, moe_route_hidden
    if path not in ("fused", "native"):
        raise RuntimeError("path must be 'fused' or 'native'")
    if "return_keys" in routing:
        raise RuntimeError("fp4_moe_routed returns the layer's output only: call moe_route(..., return_keys=True) for the keys")
    if path == "fused":
        _check_fused(kind, activation)
        if transient:
            raise RuntimeError("transient=True is for path 'native'")
    else:
        _check_native(kind, activation, activations, transient)
    _check_invariant_layer(invariant, path, kind, hidden)
    if router_weight is not None:
        if router_logits is not None:
            raise RuntimeError("router_logits must be None when router_weight is given: the layer then starts at the hidden state")
        if router_weight.dim() != 2:
            raise RuntimeError("router_weight must be [num_experts, k]")
        global_experts = router_weight.size(0)
    else:
        if router_bias is not None or router_input is not None:
            raise RuntimeError("router_bias and router_input need router_weight")
        if router_logits is None or router_logits.dim() != 2 or router_logits.size(0) != hidden.size(0):
            raise RuntimeError(f"router_logits must be [{hidden.size(0)}, num_experts] (tokens of hidden)")
        global_experts = router_logits.size(1)
    num_shared = int(routing.get("num_shared", 0))
    if routing.get("expert_map") is None:
        local = global_experts
    else:
        given = routing.get("num_local_experts")
        local = global_experts if given is None or int(given) <= 0 else int(given)
    if gs13.numel() != local + num_shared:
        raise RuntimeError(f"the weights hold {gs13.numel()} experts, the routing names {local} local + {num_shared} shared "
                           f"(router_logits must be [{hidden.size(0)}, {gs13.numel() - num_shared}] without an expert_map)")
    norm = _norm_end(norm_weight, norm_eps, norm_residual, norm_weight_offset, norm_fmt)
    if router_weight is not None:
        w, ids, sorted_pos, offsets, token_index = moe_route_hidden(router_input if router_input is not None else hidden, router_weight, topk,
                                                                    router_bias=router_bias, **routing)
    else:
        w, ids, sorted_pos, offsets, token_index = moe_route_align(router_logits, topk, **routing)
    if path == "fused":
        return _fused_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, kind, bias13, bias2, activation,
                                  norm, invariant)
    return _native_after_align(hidden, w13, s13, gs13, w2, s2, gs2, w, ids, sorted_pos, offsets, token_index, kind, activations, bias13, bias2,
                               activation, transient, norm)

"""Host side of the encoder's positional input (include/posembed.h): the sine embedding of the padding
masks -- DeVIS's ``PositionEmbeddingSine`` -- as ``[N, C, H, W]`` of one level, or for all levels at once in the layout the
encoder reads, ``[N, sum HW, C]`` with the temporal and the level embedding added, together with the flattened masks and the
valid ratios (the positional part of ``DeformableTransformer.prepare_data``).  Argument checks, the output and workspace
tensors, and the kernel launches: a counts pass and a write pass for the forward, a partial and a combine pass for the
backward.  The custom ops of :mod:`devis_amd.ops` run exactly this code.

Nothing here reads a device value on the host.  The backward has no atomics: the gradients of the two embeddings are bitwise
reproducible, and nothing here raises or warns under ``torch.use_deterministic_algorithms(True)``.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import math

import torch

from .. import _native, _posembed
from ._common import _check_device, _require, eager_backward

OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
ROUND_DTYPES = (torch.bfloat16, torch.float16)


def check_features(op, num_pos_feats, normalize, scale):
    """The reference constructor's rules, and the one its ``stack`` of the sine and cosine halves implies.  Returns the
    scale the kernels get (``2 * pi`` when none is given)."""
    _require(isinstance(num_pos_feats, int) and num_pos_feats > 0 and num_pos_feats % 2 == 0,
             "%s: num_pos_feats must be even and positive, got %s" % (op, num_pos_feats))
    if scale is not None and not normalize:
        raise ValueError("normalize should be True if scale is passed")
    return 2 * math.pi if scale is None else float(scale)


def check_masks(op, masks):
    """Shape and dtype contract of the masks; works on fake tensors.  Returns (N, [(H, W), ...])."""
    _require(1 <= len(masks) <= _posembed.MAX_LEVELS, "%s: 1 to %d levels, got %d" % (op, _posembed.MAX_LEVELS, len(masks)))
    for l, m in enumerate(masks):
        _require(m.dtype == torch.bool, "%s: the mask of level %d must be bool, got %s" % (op, l, m.dtype))
        _require(m.dim() == 3, "%s: the mask of level %d must be [N, H, W]" % (op, l))
        _require(m.shape[0] == masks[0].shape[0], "%s: the mask of level %d has %s frames, level 0 %s"
                 % (op, l, m.shape[0], masks[0].shape[0]))
        _require(m.shape[1] > 0 and m.shape[2] > 0, "%s: the mask of level %d is empty" % (op, l))
    return masks[0].shape[0], [(m.shape[1], m.shape[2]) for m in masks]


def check_encoder(masks, level_embed, temporal_embed, num_pos_feats, normalize, scale, round_dtype, out_dtype):
    """Contract of encoder_position_embedding; raises before anything is launched.  Works on fake tensors.  Returns
    (N, sizes, C, num_pos_feats, scale, out_dtype)."""
    op = "encoder_position_embedding"
    N, sizes = check_masks(op, masks)
    _require(level_embed.dim() == 2 and level_embed.is_floating_point(), "%s: level_embed must be a floating [L, C] tensor" % op)
    _require(level_embed.shape[0] == len(masks), "%s: %d masks, but level_embed has %s levels" % (op, len(masks), level_embed.shape[0]))
    C = level_embed.shape[1]
    num_pos_feats = C // 2 if num_pos_feats is None else num_pos_feats
    scale = check_features(op, num_pos_feats, normalize, scale)
    _require(C == 2 * num_pos_feats, "%s: level_embed has %s channels, 2 * num_pos_feats is %s" % (op, C, 2 * num_pos_feats))
    if temporal_embed is not None:
        _require(temporal_embed.dim() == 2 and temporal_embed.is_floating_point(), "%s: temporal_embed must be a floating [N, C] tensor" % op)
        _require(temporal_embed.shape[0] == N, "%s: temporal_embed has %s frames, the masks %s" % (op, temporal_embed.shape[0], N))
        _require(temporal_embed.shape[1] == C, "%s: temporal_embed has %s channels, level_embed %s" % (op, temporal_embed.shape[1], C))
    _require(round_dtype is None or round_dtype in ROUND_DTYPES, "%s: round_dtype must be bfloat16, float16 or None" % op)
    if out_dtype is None:
        out_dtype = torch.promote_types(round_dtype or torch.float32, level_embed.dtype)
    _require(out_dtype in OUT_DTYPES, "%s: out_dtype must be float32, bfloat16 or float16, got %s" % (op, out_dtype))
    return N, sizes, C, num_pos_feats, scale, out_dtype


def check_sine(mask, num_pos_feats, normalize, scale, out_dtype):
    """Contract of sine_position_embedding.  Returns (N, (H, W), scale, out_dtype)."""
    op = "sine_position_embedding"
    scale = check_features(op, num_pos_feats, normalize, scale)
    N, sizes = check_masks(op, [mask])
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    _require(out_dtype in OUT_DTYPES, "%s: out_dtype must be float32, bfloat16 or float16, got %s" % (op, out_dtype))
    return N, sizes[0], scale, out_dtype


_dim_t = {}         # (num_pos_feats, temperature, device) -> the reference's table (a few hundred bytes each)


def dim_t_of(num_pos_feats, temperature, device):
    """``dim_t`` [num_pos_feats] float32 built with the reference's expression (position_encoding.py:90-91) on ``device``: its
    table bit for bit.  One tensor per (size, temperature, device); not kept when built inside a HIP-graph capture."""
    key = (num_pos_feats, temperature, str(device))
    hit = _dim_t.get(key)
    if hit is None:
        hit = torch.arange(num_pos_feats, dtype=torch.float32, device=device)
        hit = temperature ** (2 * (torch.div(hit, 2, rounding_mode='trunc')) / num_pos_feats)
        if not (hit.is_cuda and torch.cuda.is_current_stream_capturing()):
            if len(_dim_t) >= 32:
                _dim_t.clear()
            _dim_t[key] = hit
    return hit


def _run_counts(masks, N, sizes, with_flat):
    """The counts pass.  Returns (workspace, mask_flatten bool [N, S] or None, valid_ratios [N, L, 2] or None)."""
    dev = masks[0].device
    S = sum(h * w for h, w in sizes)
    shape = _posembed.shape_of(N, sizes, 0)
    workspace = torch.empty(_posembed.workspace_bytes(_posembed.WS_COUNTS, shape), dtype=torch.uint8, device=dev)
    mask_flatten = torch.empty((N, S), dtype=torch.bool, device=dev) if with_flat else None
    valid_ratios = torch.empty((N, len(sizes), 2), dtype=torch.float32, device=dev) if with_flat else None
    if N:
        _posembed.counts(masks, shape, workspace, mask_flatten, valid_ratios)
    return workspace, mask_flatten, valid_ratios


def counts(masks):
    """What the counts pass leaves, for inspection: ``(cy [N, S], cx [N, S], ty [N, sum W], tx [N, sum H])`` int32 -- the
    cumulative sums of ``~mask`` down the columns and along the rows, and their totals -- plus ``mask_flatten`` and
    ``valid_ratios``."""
    N, sizes = check_masks("position embedding counts", masks)
    _check_device("position embedding counts", [("masks[%d]" % l, m) for l, m in enumerate(masks)])
    workspace, mask_flatten, valid_ratios = _run_counts(masks, N, sizes, True)
    S, SW, SH = sum(h * w for h, w in sizes), sum(w for _, w in sizes), sum(h for h, _ in sizes)
    words, at, out = workspace.view(torch.int32), 0, []
    for n in (N * S, N * S, N * SW, N * SH):
        out.append(words[at:at + n].view(N, -1))
        at += (n * 4 + 255) // 256 * 64
    return tuple(out) + (mask_flatten, valid_ratios)


def _sine(mask, num_pos_feats, temperature, normalize, scale, out_dtype):
    """pos [N, 2 * num_pos_feats, H, W]: ``PositionEmbeddingSine.forward`` of the mask."""
    N, (H, W), scale, out_dtype = check_sine(mask, num_pos_feats, normalize, scale, out_dtype)
    _check_device("sine_position_embedding", [("mask", mask)])
    C = 2 * num_pos_feats
    pos = torch.empty((N, C, H, W), dtype=out_dtype, device=mask.device)
    if N:
        workspace, _, _ = _run_counts([mask], N, [(H, W)], False)
        _posembed.write_nchw(_native.dtype_code(out_dtype), workspace, _posembed.shape_of(N, [(H, W)], C),
                             dim_t_of(num_pos_feats, temperature, mask.device), normalize, scale, pos)
    return pos


def _encoder(masks, level_embed, temporal_embed, num_pos_feats, temperature, normalize, scale, round_dtype, out_dtype):
    """(pos [N, S, C], mask_flatten bool [N, S], valid_ratios float32 [N, L, 2])."""
    N, sizes, C, num_pos_feats, scale, out_dtype = check_encoder(masks, level_embed, temporal_embed, num_pos_feats, normalize,
                                                                 scale, round_dtype, out_dtype)
    _check_device("encoder_position_embedding", [("masks[%d]" % l, m) for l, m in enumerate(masks)] +
                  [("level_embed", level_embed), ("temporal_embed", temporal_embed)])
    dev = masks[0].device
    workspace, mask_flatten, valid_ratios = _run_counts(masks, N, sizes, True)
    pos = torch.empty((N, mask_flatten.shape[1], C), dtype=out_dtype, device=dev)
    if N:
        level = level_embed.detach().float().contiguous()
        temporal = None if temporal_embed is None else temporal_embed.detach().float().contiguous()
        round_code = _posembed.NO_ROUNDING if round_dtype is None else _native.dtype_code(round_dtype)
        _posembed.write_flat(_native.dtype_code(out_dtype), workspace, _posembed.shape_of(N, sizes, C),
                             dim_t_of(num_pos_feats, temperature, dev), level, temporal, normalize, scale, round_code, pos)
    return pos, mask_flatten, valid_ratios


def _encoder_backward(grad, heights, widths, want_level, want_temporal):
    """(grad_level_embed float32 [L, C], grad_temporal_embed float32 [N, C]) of ``grad`` [N, S, C]; the one that is not wanted
    is an empty tensor and costs nothing."""
    op = "encoder_position_embedding"
    _require(grad.dim() == 3 and grad.dtype in OUT_DTYPES, "%s: the gradient of pos must be [N, S, C] in float32, bfloat16 or float16" % op)
    _check_device(op, [("grad", grad)])
    sizes = list(zip(heights, widths))
    N, S, C = grad.shape
    _require(S == sum(h * w for h, w in sizes), "%s: the gradient of pos has %s tokens, the levels %s" % (op, S, sum(h * w for h, w in sizes)))
    _require(want_level or want_temporal, "%s: no gradient is asked for" % op)
    dev = grad.device
    grad_level = torch.empty((len(sizes), C) if want_level else (0,), dtype=torch.float32, device=dev)
    grad_temporal = torch.empty((N, C) if want_temporal else (0,), dtype=torch.float32, device=dev)
    shape = _posembed.shape_of(N, sizes, C)
    workspace = torch.empty(_posembed.workspace_bytes(_posembed.WS_BACKWARD, shape), dtype=torch.uint8, device=dev)
    _posembed.backward(_native.dtype_code(grad.dtype), grad.contiguous(), shape, workspace, grad_level if want_level else None,
                       grad_temporal if want_temporal else None)
    return grad_level, grad_temporal


def setup_context(ctx, inputs, output):
    masks, level_embed, temporal_embed = inputs[:3]
    ctx.heights, ctx.widths = [m.shape[1] for m in masks], [m.shape[2] for m in masks]
    ctx.dtypes = (level_embed.dtype, None if temporal_embed is None else temporal_embed.dtype)
    ctx.mark_non_differentiable(output[1], output[2])


def backward(run, ctx, grad_pos, grad_mask, grad_ratios, embeds_at=1):
    """The autograd formula, for the op's argument order; ``run`` is :func:`_encoder_backward` or the backward op.
    ``embeds_at``: where ``level_embed`` sits among the arguments, ``temporal_embed`` following it (1 for the op)."""
    needs = ctx.needs_input_grad
    want_level, want_temporal = needs[embeds_at], needs[embeds_at + 1] and ctx.dtypes[1] is not None
    grads = [[None] * len(n) if isinstance(n, list) else None for n in needs]      # (the op's list of masks: a list of None)
    if want_level or want_temporal:
        grad_level, grad_temporal = run(grad_pos, ctx.heights, ctx.widths, want_level, want_temporal)
        grads[embeds_at] = grad_level.to(ctx.dtypes[0]) if want_level else None
        grads[embeds_at + 1] = grad_temporal.to(ctx.dtypes[1]) if want_temporal else None
    return tuple(grads)


class EncoderPositionEmbeddingFunction(torch.autograd.Function):
    """``encoder_position_embedding`` for eager code: ``apply(level_embed, temporal_embed or None, num_pos_feats, temperature,
    normalize, scale, round_dtype, out_dtype, *masks)`` -> (pos, mask_flatten, valid_ratios).  Only ``pos`` is
    differentiable, and only with respect to the two embeddings; the backward computes the gradients autograd asks for, and
    launches nothing when it asks for none."""

    # The index adapter: ``apply`` takes the masks last and one by one, since a Function does not see tensors inside a list,
    # while the formula is written for the op's arguments (``masks`` as a list, first).  forward and setup_context move them to
    # the front; the backward is told that the embeddings sit at argument 0 here, not 1.

    @staticmethod
    def forward(*args):
        return _encoder(list(args[8:]), *args[:8])

    @staticmethod
    def setup_context(ctx, inputs, output):
        setup_context(ctx, (inputs[8:],) + inputs[:8], output)

    backward = eager_backward(backward, _encoder_backward, embeds_at=0)

"""The reference's position encoding restated in plain torch, in any dtype (test infrastructure): ``PositionEmbeddingSine`` /
``PositionEmbeddingSineWithLearnableTemporal`` (src/models/position_encoding.py:78-124), the ``.to(dtype)`` of their callers
and the positional tail of ``DeformableTransformer.prepare_data`` with ``get_valid_ratio`` (deformable_transformer.py:60-94).
In float64 it is the oracle the kernels are held to; in float32 on the CPU it is the yardstick: the stock formulation's own
deviation from the oracle sets the kernels' bound (tests/test_posembed_gpu.py)."""
import math

import torch

F64 = torch.float64


def counts(mask):
    """(cy, cx, ty, tx): the integer cumulative sums of ``~mask`` [N, H, W] down the columns and along the rows, int64, and
    their totals [N, W] / [N, H]."""
    not_mask = ~mask
    cy, cx = not_mask.cumsum(1), not_mask.cumsum(2)
    return cy, cx, cy[:, -1, :], cx[:, :, -1]


def sine(mask, num_pos_feats, temperature=10000, normalize=False, scale=None, dtype=F64):
    """``PositionEmbeddingSine.forward``: [N, 2 * num_pos_feats, H, W] in ``dtype``."""
    if scale is not None and normalize is False:
        raise ValueError("normalize should be True if scale is passed")
    scale = 2 * math.pi if scale is None else scale
    open_pixels = ~mask
    halves = []
    for axis in (1, 2):                     # y, then x
        halves.append(_half(open_pixels.cumsum(axis, dtype=dtype), axis, num_pos_feats, temperature, normalize, scale))
    return torch.cat(halves, dim=3).permute(0, 3, 1, 2)


def _half(coordinate, axis, num_pos_feats, temperature, normalize, scale):
    """One half of the channels, [N, H, W, num_pos_feats]: the (normalised) running count along ``axis`` over the table of
    periods, its sine on the even and its cosine on the odd entries."""
    if normalize:
        last = coordinate.narrow(axis, coordinate.shape[axis] - 1, 1)
        coordinate = coordinate / (last + 1e-6) * scale
    k = torch.arange(num_pos_feats, dtype=coordinate.dtype, device=coordinate.device)
    periods = temperature ** (2 * (torch.div(k, 2, rounding_mode='trunc')) / num_pos_feats)
    angle = coordinate[..., None] / periods
    return torch.stack((angle[..., 0::2].sin(), angle[..., 1::2].cos()), dim=-1).flatten(-2)


def valid_ratio(mask):
    """``DeformableTransformer.get_valid_ratio``: float32 [N, 2], (w, h)."""
    open_pixels = ~mask
    rows, cols = open_pixels[:, :, 0].sum(1), open_pixels[:, 0, :].sum(1)      # down column 0, along row 0
    return torch.stack([cols.float() / mask.shape[2], rows.float() / mask.shape[1]], -1)


def encoder(masks, level_embed, temporal_embed=None, num_pos_feats=None, temperature=10000, normalize=True, scale=None,
            round_dtype=None, dtype=F64):
    """The positional results of ``prepare_data``: (lvl_pos_embed_flatten [N, S, C], mask_flatten [N, S], valid_ratios
    [N, L, 2]).  The sine part is computed in ``dtype``; the embeddings are added as they are given (cast them for the
    oracle); ``round_dtype`` is the ``.to(dtype)`` between the two additions."""
    num_pos_feats = level_embed.shape[1] // 2 if num_pos_feats is None else num_pos_feats
    embeds = []
    for lvl, mask in enumerate(masks):
        pos = sine(mask, num_pos_feats, temperature, normalize, scale, dtype)
        if temporal_embed is not None:
            pos = pos + temporal_embed[:, :, None, None]
        if round_dtype is not None:
            pos = pos.to(round_dtype)
        embeds.append(pos.flatten(2).transpose(1, 2) + level_embed[lvl].view(1, 1, -1))
    return (torch.cat(embeds, 1), torch.cat([m.flatten(1) for m in masks], 1), torch.stack([valid_ratio(m) for m in masks], 1))


def flat_sine(masks, num_pos_feats, temperature=10000, normalize=True, scale=None, dtype=F64):
    """The sine part alone in the encoder's layout: [N, S, C]."""
    return torch.cat([sine(m, num_pos_feats, temperature, normalize, scale, dtype).flatten(2).transpose(1, 2) for m in masks], 1)


def embed_rounded(sine_flat, sizes, level_embed, temporal_embed, round_dtype, out_dtype):
    """The kernels' arithmetic after the sine values, on float32 ``sine_flat`` [N, S, C]: ``+ temporal_embed[n]``, one
    rounding to ``round_dtype`` (where given), ``+ level_embed[l]`` in float32, one rounding to ``out_dtype``."""
    v = sine_flat.float()
    if temporal_embed is not None:
        v = v + temporal_embed.float()[:, None, :]
    if round_dtype is not None:
        v = v.to(round_dtype).float()
    levels = torch.cat([level_embed.float()[l].expand(h * w, -1) for l, (h, w) in enumerate(sizes)], 0)
    return (v + levels[None]).to(out_dtype)


def embedding_gradients(grad, sizes):
    """(grad_level_embed [L, C], grad_temporal_embed [N, C]) of ``grad`` [N, S, C], in grad's dtype: plain sums."""
    at, per_level = 0, []
    for h, w in sizes:
        per_level.append(grad[:, at:at + h * w].sum(1))         # [N, C]
        at += h * w
    per_level = torch.stack(per_level, 1)                       # [N, L, C]
    return per_level.sum(0), per_level.sum(1)

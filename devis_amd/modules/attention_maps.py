"""``MultiScaleMHAttentionMap``: the attention maps of DeVIS's mask head (reference ``src/models/deformable_segmentation.py``,
class of the same name) on :func:`devis_amd.ops.attention_maps` instead of einsum, masked_fill and softmax.

Same constructor, same parameter names (``q_linear``, ``k_linear``, ``q_linear_1``, ``k_linear_1``, ...) and the same
initialisation (xavier weights, zero biases), so reference checkpoints load with ``strict=True`` in both directions.  The two
projections of a level stay GEMMs through torch; the fused operator replaces everything after them.
"""
import torch
from torch import nn

from .. import ops


class MultiScaleMHAttentionMap(nn.Module):

    def __init__(self, query_dim, hidden_dim, num_heads, num_levels, dropout=0, bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.num_levels = num_levels
        self.hidden_dim = hidden_dim
        self.dropout = nn.Dropout(dropout)      # (the reference builds it and never applies it)
        for i in range(num_levels):
            for name in ("q_linear", "k_linear"):
                layer = nn.Linear(query_dim, hidden_dim, bias=bias)
                if bias:
                    nn.init.zeros_(layer.bias)
                nn.init.xavier_uniform_(layer.weight)
                setattr(self, name + self._suffix(i), layer)
        self.normalize_fact = float(hidden_dim / self.num_heads) ** -0.5

    @staticmethod
    def _suffix(i):
        return "" if i == 0 else "_%d" % i

    def _check_input(self, k, mask):
        assert len(k) == self.num_levels
        if mask is not None:
            assert len(mask) == self.num_levels

    def forward(self, q, k, mask=None):
        """``q`` [B, Q, query_dim], ``k`` a list of per-level [B, query_dim, H, W] (any strides), ``mask`` None or a list of
        per-level bool [B, H, W] -> a list of [B, Q, n, H, W]."""
        self._check_input(k, mask)
        autocast = q.is_cuda and torch.is_autocast_enabled("cuda")
        maps = []
        for i, k_lvl in enumerate(k):
            q_linear, k_linear = getattr(self, "q_linear" + self._suffix(i)), getattr(self, "k_linear" + self._suffix(i))
            B, _, H, W = k_lvl.shape
            q_lvl = q_linear(q)
            k_lvl = torch.matmul(k_linear.weight, k_lvl.flatten(2))
            if k_linear.bias is not None:
                k_lvl = k_lvl + k_linear.bias.to(k_lvl.dtype).unsqueeze(-1)
            out_dtype = None
            if autocast:
                # autocast does not reach into a custom op: hand the operator 16-bit q and k, and ask for the float32 maps
                # eager PyTorch returns there (softmax autocasts to float32)
                dt = torch.get_autocast_dtype("cuda")
                q_lvl, k_lvl, out_dtype = q_lvl.to(dt), k_lvl.to(dt), torch.float32
            maps.append(ops.attention_maps(q_lvl, k_lvl.view(B, self.hidden_dim, H, W), None if mask is None else mask[i],
                                           num_heads=self.num_heads, scale=self.normalize_fact, out_dtype=out_dtype))
        return maps

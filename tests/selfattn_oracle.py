"""Oracle of the decoder's query self-attention (include/selfattn.h): the operator and its three gradients in float64 torch,
with the mask rule of the header restated on the generator of tests/addnorm_oracle.py.  tests/ only."""
import math

import numpy as np
import torch

from addnorm_oracle import MASK32, philox4x32_10, scale_of, threshold_of  # noqa: F401  (scale_of: for the callers)


def keep_mask(seed, N, H, L, S, p):
    """bool [N, H, L, S]: probability (n, h, i, j) is kept iff word (j & 3) of Philox4x32-10(key = (seed low, seed high),
    counter = (row low, row high, j >> 2, 1)) with row = (n * H + h) * L + i is >= floor(p * 2^32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rows = np.arange(N * H * L, dtype=np.uint64)[:, None]
    quads = np.arange((S + 3) // 4, dtype=np.uint64)[None, :]
    words = philox4x32_10((rows & np.uint64(MASK32), rows >> np.uint64(32), quads, 1), (seed & MASK32, seed >> 32))
    words = np.stack([np.broadcast_to(w, (N * H * L, quads.shape[1])) for w in words], -1).reshape(N * H * L, -1)[:, :S]
    return torch.from_numpy(words >= np.uint64(threshold_of(p))).view(N, H, L, S)


def attention(q, k, v, num_heads, keep=None, scale=1.0):
    """float64 ``out [L, N, E]``: q [L, N, E], k and v [S, N, E]; ``keep`` [N, H, L, S] bool or None."""
    q, k, v = (t.double() for t in (q, k, v))
    L, N, E = q.shape
    S, H = k.shape[0], num_heads
    D = E // H
    heads = lambda t, rows: t.reshape(rows, N, H, D).permute(1, 2, 0, 3)      # noqa: E731  [N, H, rows, D]
    logits = heads(q, L) @ heads(k, S).transpose(-1, -2) / math.sqrt(D)
    prob = torch.softmax(logits, -1) * scale
    if keep is not None:
        prob = torch.where(keep.to(prob.device), prob, torch.zeros_like(prob))
    return (prob @ heads(v, S)).permute(2, 0, 1, 3).reshape(L, N, E)


def attention_grads(q, k, v, num_heads, grad_out, keep=None, scale=1.0):
    """(out, grad_q, grad_k, grad_v) in float64."""
    leaves = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    out = attention(*leaves, num_heads, keep, scale)
    return (out.detach(),) + torch.autograd.grad(out, leaves, grad_out.double())

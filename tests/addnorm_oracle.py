"""Oracle of the transformer layers' glue operators (include/addnorm.h): Philox4x32-10 in numpy, the mask rule of the header
restated, and the two operators with their gradients in float64 torch, given that mask.  tests/ only."""
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """The four output words of Philox4x32-10.  ``counter``: four uint32 arrays (or ints) that broadcast, ``key``: two.
    Returns a list of four uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    k = [int(v) & MASK32 for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # 32 x 32 -> 64 bits: no overflow
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
        k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
    return c


def threshold_of(p):
    return int(math.floor(float(p) * 4294967296.0))


def scale_of(p):
    return 1.0 / (1.0 - float(p)) if p < 1.0 else 0.0


def keep_mask(seed, R, C, p):
    """bool [R, C]: element (row, c) is kept iff word (c & 3) of Philox4x32-10(key = (seed low, seed high), counter = (row low,
    row high, c >> 2, 0)) is >= floor(p * 2^32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rows = np.arange(R, dtype=np.uint64)[:, None]
    quads = np.arange((C + 3) // 4, dtype=np.uint64)[None, :]
    words = philox4x32_10((rows & np.uint64(MASK32), rows >> np.uint64(32), quads, 0), (seed & MASK32, seed >> 32))
    words = np.stack([np.broadcast_to(w, (R, quads.shape[1])) for w in words], -1).reshape(R, -1)[:, :C]
    return torch.from_numpy(words >= np.uint64(threshold_of(p)))


def add_layer_norm(x, delta, weight, bias, eps, keep=None, scale=1.0):
    """float64 ``LayerNorm(x + dropout(delta))`` over the last dimension, the mask ``keep`` (x's shape, or None) given."""
    x, delta, weight, bias = (t.double() for t in (x, delta, weight, bias))
    d = delta * scale
    if keep is not None:
        d = torch.where(keep.to(d.device).view(x.shape), d, torch.zeros_like(d))
    z = x + d
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * weight + bias


def add_layer_norm_grads(x, delta, weight, bias, eps, grad_y, keep=None, scale=1.0):
    """(y, grad_x, grad_delta, grad_weight, grad_bias) in float64."""
    leaves = [t.detach().double().requires_grad_(True) for t in (x, delta, weight, bias)]
    y = add_layer_norm(*leaves, eps, keep, scale)
    return (y.detach(),) + torch.autograd.grad(y, leaves, grad_y.double())


def relu_dropout(x, keep=None, scale=1.0):
    y = torch.relu(x.double()) * scale
    if keep is not None:
        y = torch.where(keep.to(y.device).view(x.shape), y, torch.zeros_like(y))
    return y


def relu_dropout_grad(x, grad_y, keep=None, scale=1.0):
    leaf = x.detach().double().requires_grad_(True)
    return torch.autograd.grad(relu_dropout(leaf, keep, scale), leaf, grad_y.double())[0]

"""Oracle of the Swin backbone's (shifted-)window attention (tests/ only), written from the rule of include/winattn.h and not
from the kernels: the literal chain -- roll by -shift, partition into windows, scaled logits, relative-position bias gathered
from the table, shift mask, softmax, product with v, reverse the partition, roll by +shift -- in torch, in the dtype of its
operands (the tests pass float64), with all gradients by autograd.  The mask comes from the header's region rule
(:func:`shift_mask`); :func:`sliced_mask` paints the regions with slices instead, as the reference's ``BasicLayer.forward`` does,
and the CPU tests compare the two."""
import functools

import torch

MASKED = -100.0


@functools.lru_cache(maxsize=None)
def relative_rows(ws):
    """[N, N]: the table row of (query token i, key token j): (iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1).  Callers do
    not write to the result."""
    rows = torch.empty(ws * ws, ws * ws, dtype=torch.int64)
    for i in range(ws * ws):
        for j in range(ws * ws):
            rows[i, j] = (i // ws - j // ws + ws - 1) * (2 * ws - 1) + (i % ws - j % ws + ws - 1)
    return rows


def band(c, n, ws, shift):
    """r(c, n) = (c >= n - ws) + (c >= n - shift)."""
    return int(c >= n - ws) + int(c >= n - shift)


def region_map(Hp, Wp, ws, shift):
    """[Hp, Wp]: region = 3 r(ys, Hp) + r(xs, Wp) at the shifted coordinates (ys, xs)."""
    return torch.tensor([[3 * band(ys, Hp, ws, shift) + band(xs, Wp, ws, shift) for xs in range(Wp)] for ys in range(Hp)])


def partition(x, ws):
    """[B, Hp, Wp, ...] -> [B, nW, N, ...]: window w = wy * (Wp / ws) + wx, token i = iy * ws + ix."""
    B, Hp, Wp = x.shape[:3]
    rest = tuple(x.shape[3:])
    x = x.reshape((B, Hp // ws, ws, Wp // ws, ws) + rest)
    order = (0, 1, 3, 2, 4) + tuple(range(5, 5 + len(rest)))
    return x.permute(order).reshape((B, (Hp // ws) * (Wp // ws), ws * ws) + rest)


def reverse(windows, ws, Hp, Wp):
    """[B, nW, N, ...] -> [B, Hp, Wp, ...]: the inverse of :func:`partition`."""
    B = windows.shape[0]
    rest = tuple(windows.shape[3:])
    x = windows.reshape((B, Hp // ws, Wp // ws, ws, ws) + rest)
    order = (0, 1, 3, 2, 4) + tuple(range(5, 5 + len(rest)))
    return x.permute(order).reshape((B, Hp, Wp) + rest)


def mask_of_regions(regions, ws):
    """[Hp, Wp] region numbers -> [nW, N, N]: -100 where the regions of query and key differ, else 0."""
    per_window = partition(regions[None], ws)[0]                         # [nW, N]
    differ = per_window[:, :, None] != per_window[:, None, :]
    return differ.double() * MASKED


def shift_mask(Hp, Wp, ws, shift):
    """mask(i, j) of every window by the header's rule; None without a shift."""
    return mask_of_regions(region_map(Hp, Wp, ws, shift), ws) if shift else None


def sliced_mask(Hp, Wp, ws, shift):
    """The same mask with the nine regions painted by slices ([0, -ws), [-ws, -shift), [-shift, end) in both directions and
    numbered row-major), the way the reference's BasicLayer.forward builds it.  shift > 0."""
    regions = torch.zeros(Hp, Wp, dtype=torch.int64)
    cuts = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    for number, (rows, cols) in enumerate((r, c) for r in cuts for c in cuts):
        regions[rows, cols] = number
    return mask_of_regions(regions, ws)


def attention(qkv, table, num_heads, ws, shift=0, scale=None):
    """out [B, Hp, Wp, C] of qkv [B, Hp, Wp, 3C] and table [(2 ws - 1)^2, nH], in their dtype."""
    B, Hp, Wp, C3 = qkv.shape
    H, C = num_heads, C3 // 3
    D, N = C // H, ws * ws
    scale = D ** -0.5 if scale is None else scale
    rolled = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    windows = partition(rolled.reshape(B, Hp, Wp, 3, H, D), ws)           # [B, nW, N, 3, H, D]
    q, k, v = (windows[:, :, :, part].transpose(2, 3) for part in range(3))   # [B, nW, H, N, D]
    logits = scale * (q @ k.transpose(-1, -2))
    bias = table[relative_rows(ws).reshape(-1)].reshape(N, N, H).permute(2, 0, 1)      # [H, N, N]
    logits = logits + bias.to(logits.dtype)
    if shift:
        logits = logits + shift_mask(Hp, Wp, ws, shift).to(logits.dtype)[None, :, None]
    out = torch.softmax(logits, -1) @ v                                  # [B, nW, H, N, D]
    merged = reverse(out.transpose(2, 3).reshape(B, -1, N, C), ws, Hp, Wp)
    return torch.roll(merged, (shift, shift), (1, 2)) if shift else merged


def attention_grads(qkv, table, num_heads, ws, shift, grad_out, scale=None):
    """(out, grad_qkv, grad_table) in float64."""
    with torch.enable_grad():
        a, b = qkv.detach().double().requires_grad_(True), table.detach().double().requires_grad_(True)
        out = attention(a, b, num_heads, ws, shift, scale)
        grads = torch.autograd.grad(out, (a, b), grad_out.detach().double())
    return (out.detach(),) + grads

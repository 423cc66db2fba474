"""The rule of include/prenorm.h in float64 torch, written from the header (tests/ only): the three source forms of a row, the
norm, both destinations and every gradient by the header's formulas (no autograd), plus the header's summation order restated
in float32 numpy for the bitwise tests.  Inputs are taken as they are (the caller rounds them to the storage dtype first)."""
import numpy as np
import torch


def _rows(x, delta=None, keep=None, merge=None, s_dtype=None):
    """(z [R, C] float64, s or None): the rows a call normalises.  ``merge=(H, W)``: x is [B, H * W, Cin] and the rows are the
    2 x 2 gathers; otherwise x is [B, L, C], with ``delta`` and ``keep [B]`` the residual form.  ``s_dtype``: the storage dtype
    s is rounded to (the norm then reads the rounded s)."""
    x = x.double()
    if merge is not None:
        H, W = merge
        B, L, Cin = x.shape
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        grid = torch.zeros(B, 2 * H2, 2 * W2, Cin, dtype=torch.float64)
        grid[:, :H, :W] = x.view(B, H, W, Cin)
        z = torch.zeros(B, H2, W2, 4 * Cin, dtype=torch.float64)
        for q, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):         # the order of PatchMerging.forward
            z[..., q * Cin:(q + 1) * Cin] = grid[:, dy::2, dx::2]
        return z.reshape(-1, 4 * Cin), None
    B, C = x.shape[0], x.shape[-1]
    if delta is None:
        return x.reshape(-1, C), None
    k = torch.ones(B, dtype=torch.float64) if keep is None else keep.double()
    t = x.clone()
    for b in range(B):
        if k[b] != 0:                                        # (an entry with k == 0 takes exactly x, whatever delta holds)
            t[b] = x[b] + delta[b].double() * k[b]
    if s_dtype is not None:
        t = t.to(s_dtype).double()
    return t.reshape(-1, C), t


def _to_map(y, B, map_size):
    H, W, Hp, Wp = map_size
    out = torch.zeros(B, Hp, Wp, y.shape[-1], dtype=torch.float64)
    out[:, :H, :W] = y.view(B, H, W, -1)
    return out


def forward(x, delta, weight, bias, eps, keep=None, merge=None, map_size=None, s_dtype=None):
    """{"s", "y", "mean", "rstd"} in float64; y is [R, C], or the map [B, Hp, Wp, C] with exact zeros as padding."""
    z, s = _rows(x, delta, keep, merge, s_dtype)
    mean = z.mean(1, keepdim=True)
    var = ((z - mean) ** 2).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    y = ((z - mean) * rstd) * weight.double() + bias.double()
    if map_size is not None:
        y = _to_map(y, x.shape[0], map_size)
    return {"s": s, "y": y, "mean": mean[:, 0], "rstd": rstd[:, 0]}


def grads(x, delta, weight, bias, eps, grad_y, grad_s=None, keep=None, merge=None, map_size=None, s_dtype=None, stats=None):
    """{"grad_x", "grad_delta", "grad_weight", "grad_bias"} in float64 by the header's backward; grad_y in y's layout.
    ``stats=(mean, rstd)``: the saved statistics [R] to use instead of recomputing them (``eps`` is then not read)."""
    z, s = _rows(x, delta, keep, merge, s_dtype)
    R, C = z.shape
    B = x.shape[0]
    g = grad_y.double()
    if map_size is not None:
        H, W, Hp, Wp = map_size
        g = g[:, :H, :W]                                     # (padding positions are not read)
    g = g.reshape(R, C)
    if stats is None:
        mean = z.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt(((z - mean) ** 2).mean(1, keepdim=True) + eps)
    else:
        mean, rstd = (t.double().reshape(R, 1) for t in stats)
    xhat = (z - mean) * rstd
    gw = g * weight.double()
    c1, c2 = gw.mean(1, keepdim=True), (gw * xhat).mean(1, keepdim=True)
    dz = ((gw - c1) - xhat * c2) * rstd
    if grad_s is not None:
        dz = dz + grad_s.double().reshape(R, C)
    out = {"grad_weight": (g * xhat).sum(0), "grad_bias": g.sum(0), "grad_delta": None}
    if merge is not None:
        H, W = merge
        Cin = C // 4
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        grid = torch.zeros(B, 2 * H2, 2 * W2, Cin, dtype=torch.float64)
        dz = dz.view(B, H2, W2, C)
        for q, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            grid[:, dy::2, dx::2] = dz[..., q * Cin:(q + 1) * Cin]
        out["grad_x"] = grid[:, :H, :W].reshape(B, H * W, Cin)                  # (the gradient of padded pieces is dropped)
        return out
    out["grad_x"] = dz.view(x.shape)
    if delta is not None:
        k = torch.ones(B, dtype=torch.float64) if keep is None else keep.double()
        gd = torch.zeros(x.shape, dtype=torch.float64)
        for b in range(B):
            if k[b] != 0:
                gd[b] = out["grad_x"][b] * k[b]
        out["grad_delta"] = gd
    return out


# ---- the header's order of the sums over C, in float32 ---------------------------------------------------------------------

def row_sum_f32(v):
    """The sum over the channels of v [R, C] float32 in the header's order: lane l owns the channels (g * 64 + l) * 4 + j and
    adds them with g, then j, ascending (channels >= C as 0); butterflies xor 32, 16, .. 1."""
    v = np.asarray(v, dtype=np.float32)
    R, C = v.shape
    G = -(-C // 256)
    padded = np.zeros((R, G * 256), dtype=np.float32)
    padded[:, :C] = v
    lanes = padded.reshape(R, G, 64, 4)
    s = np.zeros((R, 64), dtype=np.float32)
    for g in range(G):
        for j in range(4):
            s = (s + lanes[:, g, :, j]).astype(np.float32)
    d = 32
    while d:
        s = (s + s[:, np.arange(64) ^ d]).astype(np.float32)
        d >>= 1
    assert (s == s[:, :1]).all() or np.isnan(s).any()
    return s[:, 0]


def mean_f32(z):
    """mean [R] of z [R, C] float32 with the kernels' bits: the ordered sum, divided by C."""
    z = np.asarray(z, dtype=np.float32)
    return (row_sum_f32(z) / np.float32(z.shape[1])).astype(np.float32)


def var_f32(z):
    """var [R] with the kernels' bits: the ordered sum of the rounded squares of the rounded differences, divided by C."""
    z = np.asarray(z, dtype=np.float32)
    t = (z - mean_f32(z)[:, None]).astype(np.float32)
    return (row_sum_f32((t * t).astype(np.float32)) / np.float32(z.shape[1])).astype(np.float32)

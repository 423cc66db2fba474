"""The rule of include/swinends.h in float64 torch, written from the header (tests/ only): the patch embedding with its norm in
token order and the output norm in NCHW, and every gradient by the header's formulas (no autograd, no convolution).  Inputs are
taken as they are (the caller rounds them to the storage dtype first)."""
import torch


def patches(image, p):
    """patch [B, Hp * Wp, K] float64 with k = (cin * p + dy) * p + dx; a pixel outside H x W is exactly 0."""
    B, Cin, H, W = image.shape
    Hp, Wp = -(-H // p), -(-W // p)
    padded = torch.zeros(B, Cin, Hp * p, Wp * p, dtype=torch.float64)
    padded[:, :, :H, :W] = image.double()
    t = padded.view(B, Cin, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5)      # b, i, j, cin, dy, dx
    return t.reshape(B, Hp * Wp, Cin * p * p)


def _project(image, proj_weight, proj_bias):
    C, p = proj_weight.shape[0], proj_weight.shape[2]
    pt = patches(image, p)
    z = pt @ proj_weight.double().reshape(C, -1).t()
    if proj_bias is not None:
        z = z + proj_bias.double()
    return pt, z


def _stats(z, eps):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1 / torch.sqrt(var + eps)


def embed_forward(image, proj_weight, proj_bias, norm_weight, norm_bias, eps=1e-5):
    """{"tokens" [B, Hp * Wp, C], "mean", "rstd" [B, Hp * Wp] (None without a norm)} in float64."""
    _, z = _project(image, proj_weight, proj_bias)
    if norm_weight is None:
        return {"tokens": z, "mean": None, "rstd": None}
    mean, rstd = _stats(z, eps)
    return {"tokens": ((z - mean) * rstd) * norm_weight.double() + norm_bias.double(), "mean": mean[..., 0], "rstd": rstd[..., 0]}


def embed_grads(image, proj_weight, proj_bias, norm_weight, eps, grad_tokens, stats=None):
    """{"grad_proj_weight", "grad_proj_bias", "grad_norm_weight", "grad_norm_bias"} in float64 by the header's backward.
    ``stats=(mean, rstd)``: the saved statistics to use instead of recomputing them."""
    pt, z = _project(image, proj_weight, proj_bias)
    g = grad_tokens.double()
    out = {"grad_norm_weight": None, "grad_norm_bias": None}
    if norm_weight is None:
        dz = g
    else:
        if stats is None:
            mean, rstd = _stats(z, eps)
        else:
            mean, rstd = (t.double().reshape(z.shape[:-1] + (1,)) for t in stats)
        xhat = (z - mean) * rstd
        gw = g * norm_weight.double()
        c1, c2 = gw.mean(-1, keepdim=True), (gw * xhat).mean(-1, keepdim=True)
        dz = ((gw - c1) - xhat * c2) * rstd
        out["grad_norm_weight"] = (g * xhat).sum((0, 1))
        out["grad_norm_bias"] = g.sum((0, 1))
    out["grad_proj_bias"] = dz.sum((0, 1))
    out["grad_proj_weight"] = torch.einsum("blc,blk->ck", dz, pt).reshape(proj_weight.shape)
    return out


def map_forward(x, H, W, weight, bias, eps=1e-5):
    """{"y" [B, C, H, W], "mean", "rstd" [B, H * W]} in float64."""
    z = x.double()
    B, L, C = z.shape
    mean, rstd = _stats(z, eps)
    y = ((z - mean) * rstd) * weight.double() + bias.double()
    return {"y": y.view(B, H, W, C).permute(0, 3, 1, 2).contiguous(), "mean": mean[..., 0], "rstd": rstd[..., 0]}


def map_grads(x, H, W, weight, eps, grad_y, stats=None):
    """{"grad_x" [B, H * W, C], "grad_weight", "grad_bias"} in float64; grad_y is [B, C, H, W]."""
    z = x.double()
    B, L, C = z.shape
    g = grad_y.double().permute(0, 2, 3, 1).reshape(B, L, C)
    if stats is None:
        mean, rstd = _stats(z, eps)
    else:
        mean, rstd = (t.double().reshape(B, L, 1) for t in stats)
    xhat = (z - mean) * rstd
    gw = g * weight.double()
    c1, c2 = gw.mean(-1, keepdim=True), (gw * xhat).mean(-1, keepdim=True)
    return {"grad_x": ((gw - c1) - xhat * c2) * rstd, "grad_weight": (g * xhat).sum((0, 1)), "grad_bias": g.sum((0, 1))}

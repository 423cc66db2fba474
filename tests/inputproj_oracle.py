"""Float64 restatement of include/inputproj.h, written from the header and not from torch's GroupNorm: the statistics of every
group, the tokens, and every gradient by the header's formulas.  Inputs are taken as they are stored (16-bit tensors are
widened exactly); results are float64 CPU tensors.
"""
import torch


def _f64(t):
    return t.detach().double().cpu()


def statistics(xs, num_groups, eps=1e-5):
    """(mean, rstd), each [N, L, G]: over the contiguous run of C / G channels x H x W elements of a group."""
    means, rstds = [], []
    for x in xs:
        x = _f64(x)
        N, C = x.shape[:2]
        runs = x.reshape(N, num_groups, -1)
        mean = runs.sum(2) / runs.shape[2]
        var = ((runs - mean[:, :, None]) ** 2).sum(2) / runs.shape[2]
        means.append(mean)
        rstds.append(1.0 / torch.sqrt(var + eps))
    return torch.stack(means, 1), torch.stack(rstds, 1)


def _xhat(x, mean, rstd, num_groups):
    N, C = x.shape[:2]
    runs = x.reshape(N, num_groups, -1)
    return ((runs - mean[:, :, None]) * rstd[:, :, None]).reshape(N, C, -1)          # [N, C, HW]


def forward(xs, num_groups, weights, biases, eps=1e-5):
    """{tokens [N, S, C], mean, rstd}: tokens[n, start_l + p, c] = xhat * weight_l[c] + bias_l[c]."""
    mean, rstd = statistics(xs, num_groups, eps)
    levels = []
    for l, (x, w, b) in enumerate(zip(xs, weights, biases)):
        xhat = _xhat(_f64(x), mean[:, l], rstd[:, l], num_groups)
        y = xhat * _f64(w)[None, :, None] + _f64(b)[None, :, None]
        levels.append(y.permute(0, 2, 1))
    return {"tokens": torch.cat(levels, 1), "mean": mean, "rstd": rstd}


def grads(xs, num_groups, weights, grad_tokens, eps=1e-5):
    """{grad_x: [..], grad_weight: [..], grad_bias: [..]} by the header's backward: the per-channel sums A and B, the group
    terms c1 and c2, and grad_x = ((g w - c1) - xhat c2) rstd."""
    mean, rstd = statistics(xs, num_groups, eps)
    g_all = _f64(grad_tokens)
    out = {"grad_x": [], "grad_weight": [], "grad_bias": []}
    start = 0
    for l, (x, w) in enumerate(zip(xs, weights)):
        x, w = _f64(x), _f64(w)
        N, C, H, W = x.shape
        cpg = C // num_groups
        g = g_all[:, start:start + H * W].permute(0, 2, 1)                          # [N, C, HW]
        start += H * W
        xhat = _xhat(x, mean[:, l], rstd[:, l], num_groups)
        A, B = g.sum(2), (g * xhat).sum(2)                                          # [N, C]
        out["grad_bias"].append(A.sum(0))
        out["grad_weight"].append(B.sum(0))
        M = cpg * H * W
        c1 = (w[None] * A).reshape(N, num_groups, cpg).sum(2) / M
        c2 = (w[None] * B).reshape(N, num_groups, cpg).sum(2) / M
        c1, c2 = (t.repeat_interleave(cpg, 1)[:, :, None] for t in (c1, c2))
        r = rstd[:, l].repeat_interleave(cpg, 1)[:, :, None]
        out["grad_x"].append((((g * w[None, :, None] - c1) - xhat * c2) * r).reshape(N, C, H, W))
    return out

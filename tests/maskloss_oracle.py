"""Float64 oracle of the mask loss (include/maskloss.h), in plain torch on the CPU: the resampling rule as explicit tap
matrices, the per-pixel focal and dice terms, and the analytic gradient of the logits.  No reference code in it; the fixtures
of tests/golden/maskloss_*.npz tie it to the reference (tests/test_maskloss_cpu.py)."""
import torch

F64 = torch.float64


def taps(size_in, size_out, arith=torch.float32, rule="half_pixel"):
    """(i0, i1, l0, l1) per destination index, each [size_out]: the header's rule evaluated in ``arith`` (float32 as the
    kernels do for every dtype but float64), the weights returned in float64.  ``rule``: "half_pixel" is the operator's;
    "align_corners" and "integer" are the wrong rules a test must tell apart."""
    d = torch.arange(size_out, dtype=arith)
    if rule == "half_pixel":
        scale = torch.tensor(float(size_in), dtype=arith) / torch.tensor(float(size_out), dtype=arith)
        r = (scale * (d + 0.5) - 0.5).clamp(min=0)
    elif rule == "align_corners":
        r = d * (float(size_in - 1) / float(max(size_out - 1, 1)))
    elif rule == "integer":
        r = torch.div(torch.arange(size_out) * size_in, size_out, rounding_mode="floor").to(arith)
    else:
        raise ValueError(rule)
    i0 = r.long().clamp(max=size_in - 1)
    i1 = i0 + (i0 < size_in - 1).long()
    l1 = (r - i0.to(arith)).to(F64)
    return i0, i1, 1 - l1, l1


def tap_matrix(size_in, size_out, arith=torch.float32, rule="half_pixel"):
    """U [size_out, size_in] float64 with x = U @ src along one axis."""
    i0, i1, l0, l1 = taps(size_in, size_out, arith, rule)
    U = torch.zeros(size_out, size_in, dtype=F64)
    rows = torch.arange(size_out)
    U.index_put_((rows, i0), l0, accumulate=True)
    U.index_put_((rows, i1), l1, accumulate=True)
    return U


def resample(src, size, arith=torch.float32, rule="half_pixel"):
    """src [N, h, w] -> [N, H, W] in float64."""
    Uy, Ux = tap_matrix(src.shape[1], size[0], arith, rule), tap_matrix(src.shape[2], size[1], arith, rule)
    return Uy @ src.to(F64) @ Ux.t()


def _target(target):
    return (target != 0).to(F64) if target.dtype in (torch.bool, torch.uint8) else target.to(F64)


def pixel_terms(x, t, alpha, gamma):
    """(focal, p, d focal / dx) per pixel, float64."""
    e = torch.exp(-x.abs())
    p = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    ce = x.clamp(min=0) - x * t + torch.log1p(e)
    m = 1 - (p * t + (1 - p) * (1 - t))
    if gamma == 0:
        mod, dmod = torch.ones_like(m), torch.zeros_like(m)
    elif gamma == 1:
        mod, dmod = m, torch.ones_like(m)
    else:
        mod, dmod = m.clamp(min=0) ** gamma, gamma * m.clamp(min=0) ** (gamma - 1)
    a = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(t)
    pq = p * (1 - p)
    return a * ce * mod, p, a * ((p - t) * mod + ce * dmod * (1 - 2 * t) * pq)


def mask_loss_terms(src, target, alpha=0.25, gamma=2.0, arith=torch.float32, rule="half_pixel", grads=None):
    """(focal [N], dice [N]) in float64; with ``grads = (grad_focal [N], grad_dice [N])`` also grad_src [N, h, w].  ``src``
    [N, h, w] is taken as it is (round it to the dtype under test first)."""
    N, h, w = src.shape
    H, W = target.shape[1:]
    P = H * W
    Uy, Ux = tap_matrix(h, H, arith, rule), tap_matrix(w, W, arith, rule)
    x = Uy @ src.to(F64) @ Ux.t()
    t = _target(target)
    fl, p, dfl = pixel_terms(x, t, alpha, gamma)
    A, B, C = (p * t).flatten(1).sum(1), p.flatten(1).sum(1), t.flatten(1).sum(1)
    focal, dice = fl.flatten(1).sum(1) / P, 1 - (2 * A + 1) / (B + C + 1)
    if grads is None:
        return focal, dice
    gf, gd = (g.to(F64).view(N, 1, 1) for g in grads)
    den, num = (B + C + 1).view(N, 1, 1), (2 * A + 1).view(N, 1, 1)
    g = gf / P * dfl + gd * (-(2 * t * den - num) / (den * den) * p * (1 - p))
    return focal, dice, Uy.t() @ g @ Ux


def mask_losses(src, target, num_boxes, alpha=0.25, gamma=2.0, arith=torch.float32, rule="half_pixel", with_grad=False):
    """The reference's pair: (loss_mask, loss_dice) = the sums of the terms over num_boxes; ``with_grad``: also the gradient
    of (loss_mask + loss_dice) with respect to src."""
    N = src.shape[0]
    if not with_grad:
        focal, dice = mask_loss_terms(src, target, alpha, gamma, arith, rule)
        return focal.sum() / num_boxes, dice.sum() / num_boxes
    ones = torch.full((N,), 1.0 / float(num_boxes), dtype=F64)
    focal, dice, grad = mask_loss_terms(src, target, alpha, gamma, arith, rule, grads=(ones, ones))
    return focal.sum() / num_boxes, dice.sum() / num_boxes, grad

"""Oracle of the criterion's matching cost and box losses (include/boxmatch.h), in plain torch on the CPU: the focal class
cost, the two L1 forms, the generalized IoU of cxcywh boxes with its 1e-6 terms, and the analytic gradient of the box losses
with torch autograd's conventions at the ties.  ``arith`` is the type everything is evaluated in (float64: the reference for
the tests; float32: what the kernels do for every dtype but float64).  No reference code in it; the fixtures of
tests/golden/boxmatch_*.npz tie it to the reference (tests/test_boxmatch_cpu.py)."""
import torch

F64 = torch.float64
EPS = 1e-6


def sigmoid(x):
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def class_cost(x, alpha=0.25):
    """cls(x) of the header: gamma 2, and 1 - p as sigmoid(-x)."""
    p, q = sigmoid(x), sigmoid(-x)
    return alpha * q * q * (-(p + 1e-8).log()) - (1 - alpha) * p * p * (-(q + 1e-8).log())


def corners(b):
    cx, cy, w, h = b.unbind(-1)
    return cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h


def giou(s, t):
    """GIoU of cxcywh boxes ``s`` and ``t`` [..., 4] (broadcast against each other), from torch operators: differentiable."""
    sx0, sy0, sx1, sy1 = corners(s)
    tx0, ty0, tx1, ty1 = corners(t)
    inter = (torch.min(sx1, tx1) - torch.max(sx0, tx0)).clamp(min=0) * (torch.min(sy1, ty1) - torch.max(sy0, ty0)).clamp(min=0)
    union = (sx1 - sx0) * (sy1 - sy0) + (tx1 - tx0) * (ty1 - ty0) - inter
    area = (torch.max(sx1, tx1) - torch.min(sx0, tx0)).clamp(min=0) * (torch.max(sy1, ty1) - torch.min(sy0, ty0)).clamp(min=0)
    return (inter + EPS) / (union + EPS) - ((area - union) + EPS) / (area + EPS)


def degenerate(b):
    x0, y0, x1, y1 = corners(b)
    return (x1 < x0) | (y1 < y0)


def match_cost(logits, boxes, tgt_labels, tgt_boxes, *, cost_class=1.0, cost_bbox=1.0, cost_giou=1.0, l1="mean", alpha=0.25,
               arith=F64):
    """(cost [L, R, T] in ``arith``, status int32 [3]) from logits [L, F, R, C], boxes [L, F, R, 4], tgt_labels int64 [T, F]
    and tgt_boxes [T, F, 4], which are taken as they are (round them to the dtype under test first)."""
    if l1 not in ("mean", "sum"):
        raise ValueError("l1 must be 'mean' or 'sum'")
    L, F, R, C = logits.shape
    T = tgt_labels.shape[0]
    x, b, g = logits.to(arith), boxes.to(arith), tgt_boxes.to(arith)
    ok = (tgt_labels >= 0) & (tgt_labels < C)                                            # [T, F]
    status = torch.tensor([int(degenerate(b).sum()), int(degenerate(g).sum()), int((~ok).sum())], dtype=torch.int32)
    if L * R * T == 0:
        return torch.empty(L, R, T, dtype=arith), torch.zeros(3, dtype=torch.int32)
    safe = torch.where(ok, tgt_labels, torch.zeros_like(tgt_labels))
    frames = torch.arange(F)[None].expand(T, F)
    picked = x[:, frames, :, safe]                                                       # [T, F, L, R]  (advanced dims first)
    cls = class_cost(picked.permute(2, 3, 0, 1), alpha)                                  # [L, R, T, F]
    cls = torch.where(ok[None, None], cls, torch.full_like(cls, float("nan")))
    bq = b.permute(0, 2, 1, 3)[:, :, None]                                               # [L, R, 1, F, 4]
    dist = (bq - g[None, None]).abs().sum(-1)                                            # [L, R, T, F]
    l1_term = dist.mean(-1) if l1 == "sum" else dist.mean(-1) / 4
    cost = cost_class * cls.mean(-1) + cost_bbox * l1_term + cost_giou * (-giou(bq, g[None, None]).mean(-1))
    return cost, status


def giou_grad(s, t):
    """(GIoU [N], d GIoU / d s [N, 4]) for rows of cxcywh boxes, analytically and with autograd's conventions: ties of max /
    min in halves, clamp(min=0) passing at 0."""
    sx0, sy0, sx1, sy1 = corners(s)
    tx0, ty0, tx1, ty1 = corners(t)
    hi = lambda a, b: (a > b).to(a) + 0.5 * (a == b).to(a)       # noqa: E731  share of max(a, b) going to a
    lo = lambda a, b: (a < b).to(a) + 0.5 * (a == b).to(a)       # noqa: E731  share of min(a, b) going to a
    sw, sh = sx1 - sx0, sy1 - sy0
    vw, vh = torch.min(sx1, tx1) - torch.max(sx0, tx0), torch.min(sy1, ty1) - torch.max(sy0, ty0)
    iw, ih = vw.clamp(min=0), vh.clamp(min=0)
    inter = iw * ih
    union = sw * sh + (tx1 - tx0) * (ty1 - ty0) - inter
    uw, uh = torch.max(sx1, tx1) - torch.min(sx0, tx0), torch.max(sy1, ty1) - torch.min(sy0, ty0)
    ew, eh = uw.clamp(min=0), uh.clamp(min=0)
    area = ew * eh
    n1, d1, n2, d2 = inter + EPS, union + EPS, (area - union) + EPS, area + EPS
    value = n1 / d1 - n2 / d2
    g_union = 1 / d2 - n1 / (d1 * d1)
    g_inter = 1 / d1 - g_union
    g_area = n2 / (d2 * d2) - 1 / d2
    g_iw, g_ih = (vw >= 0).to(s) * g_inter * ih, (vh >= 0).to(s) * g_inter * iw
    g_ew, g_eh = (uw >= 0).to(s) * g_area * eh, (uh >= 0).to(s) * g_area * ew
    gx1 = g_iw * lo(sx1, tx1) + g_ew * hi(sx1, tx1) + g_union * sh
    gx0 = -g_iw * hi(sx0, tx0) - g_ew * lo(sx0, tx0) - g_union * sh
    gy1 = g_ih * lo(sy1, ty1) + g_eh * hi(sy1, ty1) + g_union * sw
    gy0 = -g_ih * hi(sy0, ty0) - g_eh * lo(sy0, ty0) - g_union * sw
    return value, torch.stack([gx0 + gx1, gy0 + gy1, 0.5 * (gx1 - gx0), 0.5 * (gy1 - gy0)], -1)


def box_loss_terms(src, target, arith=F64, grads=None):
    """(l1 [N], giou [N]) in ``arith``; with ``grads = (grad_l1 [N], grad_giou [N])`` also grad_src [N, 4]."""
    s, t = src.to(arith), target.to(arith)
    value, d = giou_grad(s, t)
    l1, gl = (s - t).abs().sum(-1), 1 - value
    if grads is None:
        return l1, gl
    g1, gg = (g.to(arith)[:, None] for g in grads)
    return l1, gl, g1 * torch.sign(s - t) - gg * d


def box_losses(src, target, num_boxes, arith=F64, with_grad=False):
    """The reference's pair: (loss_bbox, loss_giou) = the sums of the terms over num_boxes; ``with_grad``: also the gradient
    of (loss_bbox + loss_giou) with respect to src."""
    if not with_grad:
        l1, gl = box_loss_terms(src, target, arith)
        return l1.sum() / num_boxes, gl.sum() / num_boxes
    ones = torch.full((src.shape[0],), 1.0 / float(num_boxes), dtype=arith)
    l1, gl, grad = box_loss_terms(src, target, arith, grads=(ones, ones))
    return l1.sum() / num_boxes, gl.sum() / num_boxes, grad

"""Host side of the criterion's box geometry (include/boxmatch.h): the cost matrix of the Hungarian
matchers and the two box losses of matched pairs.  Argument checks, the output tensors and the kernel launches: one for the
cost, one each for the losses' forward and backward.  The custom ops of :mod:`devis_amd.ops` run exactly this code.

Every result is one lane's loop in a fixed order -- there are no float atomics -- so costs, losses and grad_src are bitwise
reproducible and nothing here raises or warns under ``torch.use_deterministic_algorithms(True)``.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _boxmatch, _native
from ._common import _check_device, _require, eager_backward

L1 = {"mean": _boxmatch.L1_MEAN, "sum": _boxmatch.L1_SUM}


def check_l1(l1):
    if l1 not in L1:
        raise ValueError("match_cost: l1 must be 'mean' or 'sum', got %r" % (l1,))
    return l1


def check_match(logits, boxes, tgt_labels, tgt_boxes):
    """Shape and dtype contract of match_cost; raises before anything is launched.  Works on fake tensors.  Returns
    (L, F, R, T, C, the target kind of include/boxmatch.h)."""
    _require(logits.dim() == 4, "match_cost: logits must be [L, F, R, C]")
    _native.dtype_code(logits.dtype)       # raises on an unsupported dtype
    L, F, R, C = logits.shape
    _require(boxes.dim() == 4 and tuple(boxes.shape) == (L, F, R, 4),
             "match_cost: boxes must be [L, F, R, 4] beside logits [L, F, R, C], got %s beside %s" % (tuple(boxes.shape), tuple(logits.shape)))
    _require(boxes.dtype == logits.dtype, "match_cost: logits is %s, boxes is %s" % (logits.dtype, boxes.dtype))
    _require(tgt_labels.dim() == 2 and tgt_labels.dtype == torch.int64, "match_cost: tgt_labels must be int64 [T, F]")
    T = tgt_labels.shape[0]
    _require(tgt_labels.shape[1] == F, "match_cost: tgt_labels has %s frames, logits %s" % (tgt_labels.shape[1], F))
    _require(tgt_boxes.dim() == 3 and tuple(tgt_boxes.shape) == (T, F, 4),
             "match_cost: tgt_boxes must be [T, F, 4] beside tgt_labels [T, F], got %s" % (tuple(tgt_boxes.shape),))
    kind = _boxmatch.target_kind("match_cost", "tgt_boxes", logits.dtype, tgt_boxes.dtype)
    _require(F > 0 and C > 0, "match_cost: a mean over no frames or no classes (F = %s, C = %s)" % (F, C))
    return L, F, R, T, C, kind


def check_pairs(src, target):
    """The contract of box_loss_terms; returns (N, the target kind)."""
    _require(src.dim() == 2 and src.shape[1] == 4, "box_loss_terms: src_boxes must be [N, 4]")
    _native.dtype_code(src.dtype)
    _require(target.dim() == 2 and tuple(target.shape) == (src.shape[0], 4),
             "box_loss_terms: target_boxes must be [N, 4] like src_boxes, got %s beside %s" % (tuple(target.shape), tuple(src.shape)))
    return src.shape[0], _boxmatch.target_kind("box_loss_terms", "target_boxes", src.dtype, target.dtype)


def _match_cost(logits, boxes, tgt_labels, tgt_boxes, cost_class, cost_bbox, cost_giou, l1, alpha):
    """(cost [L, R, T] in the arithmetic type, status int32 [3])."""
    L, F, R, T, C, kind = check_match(logits, boxes, tgt_labels, tgt_boxes)
    check_l1(l1)
    _check_device("match_cost", [("logits", logits), ("boxes", boxes), ("tgt_labels", tgt_labels), ("tgt_boxes", tgt_boxes)])
    cost = torch.empty((L, R, T), dtype=_native.acc_dtype(logits.dtype), device=logits.device)
    if L * R * T == 0:
        return cost, torch.zeros(3, dtype=torch.int32, device=logits.device)
    status = torch.empty(3, dtype=torch.int32, device=logits.device)        # (zeroed by the call)
    _boxmatch.cost(_native.dtype_code(logits.dtype), kind, logits.contiguous(), boxes.contiguous(), tgt_labels.contiguous(),
                   tgt_boxes.contiguous(), _boxmatch.Shape(L, F, R, T, C), cost_class, cost_bbox, cost_giou, L1[l1], alpha,
                   cost, status)
    return cost, status


def _forward(src, target):
    """(l1 [N], giou [N]) in the arithmetic type: float32, float64 for float64 boxes."""
    N, kind = check_pairs(src, target)
    _check_device("box_loss_terms", [("src_boxes", src), ("target_boxes", target)])
    acc = _native.acc_dtype(src.dtype)
    l1, giou = torch.empty((N,), dtype=acc, device=src.device), torch.empty((N,), dtype=acc, device=src.device)
    if N:
        _boxmatch.loss_forward(_native.dtype_code(src.dtype), kind, src.contiguous(), target.contiguous(), N, l1, giou)
    return l1, giou


def _backward(grad_l1, grad_giou, src, target):
    """grad_src [N, 4] in src's dtype."""
    N, kind = check_pairs(src, target)
    _check_device("box_loss_terms", [("src_boxes", src), ("target_boxes", target), ("grad_l1", grad_l1), ("grad_giou", grad_giou)])
    _require(tuple(grad_l1.shape) == (N,) and tuple(grad_giou.shape) == (N,), "box_loss_terms: the gradients must be [N]")
    acc = _native.acc_dtype(src.dtype)
    grad_src = torch.empty((N, 4), dtype=src.dtype, device=src.device)
    if N:
        _boxmatch.loss_backward(_native.dtype_code(src.dtype), kind, src.contiguous(), target.contiguous(),
                                grad_l1.to(acc).contiguous(), grad_giou.to(acc).contiguous(), N, grad_src)
    return grad_src


def setup_context(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def backward(run, ctx, grad_l1, grad_giou):
    """The autograd formula; ``run`` is :func:`_backward` or the backward op."""
    if not ctx.needs_input_grad[0]:
        return None, None
    src, target = ctx.saved_tensors
    return run(grad_l1, grad_giou, src, target), None


class BoxLossTermsFunction(torch.autograd.Function):
    """``box_loss_terms`` for eager code: ``apply(src [N, 4], target [N, 4])`` -> (l1, giou).  Saves the two inputs as they
    were given.  No backward launch when src needs no gradient."""
    forward = staticmethod(_forward)
    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)

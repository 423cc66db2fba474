"""Host side of the criterion's label loss (include/labelloss.h): the target class of every query from
the matcher's index tensors as they lie, the sigmoid focal loss of all logits against those classes, and the matched queries'
top-1 count.  Argument checks, the output and workspace tensors, and the kernel launches: one for the forward (two beyond one
tile), one for the backward.  The custom ops of :mod:`devis_amd.ops` run exactly this code.

Nothing here reads a device value on the host: the validity mask is an operand, not a boolean index, and the counts stay on
the device.  Every sum has a fixed order -- there are no atomics on memory -- so the loss and grad_logits are bitwise
reproducible and nothing here raises or warns under ``torch.use_deterministic_algorithms(True)``.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import torch

from .. import _labelloss, _native
from ._common import _check_device, _require, eager_backward


def check_labels(logits, rows, labels, valid):
    """Shape and dtype contract of label_loss_terms; raises before anything is launched.  Works on fake tensors.  Returns
    (B, N, C, M)."""
    _require(logits.dim() == 3, "label_loss_terms: logits must be [B, N, C]")
    _native.dtype_code(logits.dtype)       # raises on an unsupported dtype
    B, N, C = logits.shape
    _require(rows.dim() == 1 and rows.dtype == torch.int64, "label_loss_terms: rows must be int64 [M]")
    _require(labels.dim() == 1 and labels.dtype == torch.int64, "label_loss_terms: labels must be int64 [M]")
    M = rows.shape[0]
    _require(labels.shape[0] == M, "label_loss_terms: labels has %s matches, rows %s" % (labels.shape[0], M))
    if valid is not None:
        _require(valid.dim() == 1 and valid.dtype in (torch.bool, torch.uint8), "label_loss_terms: valid must be bool or uint8 [M]")
        _require(valid.shape[0] == M, "label_loss_terms: valid has %s matches, rows %s" % (valid.shape[0], M))
    return B, N, C, M


def _forward(logits, rows, labels, valid, alpha):
    """(focal_sum [] in the arithmetic type -- float32, float64 for float64 logits --, counts int32 [4], target_classes
    int32 [B, N])."""
    B, N, C, M = check_labels(logits, rows, labels, valid)
    _check_device("label_loss_terms", [("logits", logits), ("rows", rows), ("labels", labels), ("valid", valid)])
    acc, dev = _native.acc_dtype(logits.dtype), logits.device
    if B * N * C == 0:
        return (torch.zeros((), dtype=acc, device=dev), torch.zeros(4, dtype=torch.int32, device=dev),
                torch.zeros((B, N), dtype=torch.int32, device=dev))
    focal_sum, counts = torch.empty((), dtype=acc, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    target_classes = torch.empty((B, N), dtype=torch.int32, device=dev)
    shape, code = _labelloss.Shape(B * N, C, M), _native.dtype_code(logits.dtype)
    nbytes = _labelloss.workspace_bytes(code, shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _labelloss.forward(code, logits.contiguous(), rows.contiguous(), labels.contiguous(),
                       None if valid is None else valid.contiguous(), shape, alpha, workspace, target_classes, focal_sum, counts)
    return focal_sum, counts, target_classes


def _backward(grad_sum, logits, target_classes, alpha):
    """grad_logits [B, N, C] in logits' dtype."""
    _require(logits.dim() == 3, "label_loss_terms: logits must be [B, N, C]")
    _check_device("label_loss_terms", [("logits", logits), ("target_classes", target_classes), ("grad_sum", grad_sum)])
    B, N, C = logits.shape
    _require(tuple(target_classes.shape) == (B, N) and target_classes.dtype == torch.int32,
             "label_loss_terms: target_classes must be int32 [B, N]")
    _require(grad_sum.numel() == 1, "label_loss_terms: the gradient of focal_sum must be one value")
    grad_logits = torch.empty((B, N, C), dtype=logits.dtype, device=logits.device)
    if B * N * C:
        _labelloss.backward(_native.dtype_code(logits.dtype), logits.contiguous(), target_classes.contiguous(),
                            grad_sum.to(_native.acc_dtype(logits.dtype)).contiguous(), _labelloss.Shape(B * N, C, 0), alpha,
                            grad_logits)
    return grad_logits


def setup_context(ctx, inputs, output):
    ctx.alpha = inputs[4]
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.save_for_backward(inputs[0], output[2])


def backward(run, ctx, grad_sum, grad_counts, grad_classes):
    """The autograd formula; ``run`` is :func:`_backward` or the backward op."""
    if not ctx.needs_input_grad[0]:
        return None, None, None, None, None
    logits, target_classes = ctx.saved_tensors
    return run(grad_sum, logits, target_classes, ctx.alpha), None, None, None, None


class LabelLossTermsFunction(torch.autograd.Function):
    """``label_loss_terms`` for eager code: ``apply(logits [B, N, C], rows [M], labels [M], valid or None, alpha)`` ->
    (focal_sum, counts, target_classes).  Saves the logits as they were given and target_classes; only focal_sum is
    differentiable.  No backward launch when logits needs no gradient."""
    forward = staticmethod(_forward)
    setup_context = staticmethod(setup_context)
    backward = eager_backward(backward, _backward)

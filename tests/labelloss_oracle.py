"""The definition of include/labelloss.h in float64 torch on the CPU: what tests hold the label-loss kernels to.  Mirrors the
operator's signature (devis_amd.label_loss_terms / label_losses); the gradient is the header's closed form, which
tests/test_labelloss_cpu.py checks against the reference's recorded one."""
import torch

F64 = torch.float64


def target_classes_of(R, C, rows, labels, valid=None):
    """(target_classes int32 [R], the good matches bool [M], counts[2], counts[3]): the good match with the highest m wins."""
    M = rows.shape[0]
    valid = torch.ones(M, dtype=torch.bool) if valid is None else valid.bool()
    row_ok, label_ok = (rows >= 0) & (rows < R), (labels >= 0) & (labels <= C)
    good = valid & row_ok & label_ok
    classes = torch.full((R,), C, dtype=torch.int32)
    for m in range(M):                          # ascending: a later match overwrites an earlier one
        if bool(good[m]):
            classes[int(rows[m])] = int(labels[m])
    return classes, good, int((valid & ~row_ok).sum()), int((valid & ~label_ok).sum())


def elements(x, t, alpha):
    """(focal, d focal / dx) per element, for logits x and the boolean targets t."""
    e = torch.exp(-x.abs())
    p = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    q = torch.where(x >= 0, e / (1 + e), 1 / (1 + e))
    ce = torch.where(t, -x, x).clamp(min=0) + torch.log1p(e)
    m = torch.where(t, q, p)
    tt = t.to(x.dtype)
    a = torch.where(t, torch.full_like(x, alpha), torch.full_like(x, 1 - alpha)) if alpha >= 0 else torch.ones_like(x)
    return ce * m * m * a, a * (torch.where(t, -q, p) * m * m + ce * 2 * m * (1 - 2 * tt) * p * q)


def label_loss_terms(logits, rows, labels, valid=None, *, alpha=0.25, grad_sum=None):
    """(focal_sum [] float64, counts int32 [4], target_classes int32 [B, N]) and, with ``grad_sum``, grad_logits [B, N, C]."""
    B, N, C = logits.shape
    x = logits.detach().to(F64).reshape(B * N, C)
    rows, labels = rows.cpu().long(), labels.cpu().long()
    classes, good, bad_rows, bad_labels = target_classes_of(B * N, C, rows, labels, None if valid is None else valid.cpu())
    t = torch.arange(C)[None, :] == classes[:, None]
    focal, dfocal = elements(x, t, float(alpha))
    correct = 0
    for m in torch.nonzero(good).flatten().tolist():
        row = x[int(rows[m])]
        if C and not bool(torch.isnan(row).any()):
            correct += int(int(torch.nonzero(row == row.max())[0]) == int(labels[m]))        # the lowest index on a tie
    counts = torch.tensor([int(good.sum()), correct, bad_rows, bad_labels], dtype=torch.int32)
    out = (focal.sum(), counts, classes.reshape(B, N))
    if grad_sum is not None:
        out += ((float(grad_sum) * dfocal).reshape(B, N, C),)
    return out


def label_losses(logits, rows, labels, valid, num_boxes, *, alpha=0.25, log=True):
    """{"loss_ce", "class_error"} as devis_amd.label_losses returns them; differentiable through the closed form."""
    focal_sum, counts, _, grad = label_loss_terms(logits, rows, labels, valid, alpha=alpha, grad_sum=1.0)
    if logits.requires_grad:
        focal_sum = _Sum.apply(logits, focal_sum.to(logits.dtype), grad.to(logits.dtype))
    losses = {"loss_ce": focal_sum / num_boxes}
    if log:
        matched, correct = int(counts[0]), int(counts[1])
        losses["class_error"] = torch.tensor(100 - (100 * correct / matched if matched else 0.0), dtype=focal_sum.dtype)
    return losses


class _Sum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, value, grad):
        ctx.save_for_backward(grad)
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None

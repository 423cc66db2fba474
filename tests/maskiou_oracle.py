"""Float64 oracle of the clip-stitching operators (include/maskiou.h), in plain torch on the CPU, on the resampling rule of
tests/maskloss_oracle.py (imported, not copied).  No reference code in it; the fixtures of tests/golden/maskiou_*.npz tie it
to the reference (tests/test_maskiou_cpu.py)."""
import torch

from maskloss_oracle import resample

F64 = torch.float64


def logits(src, size, arith=torch.float32):
    """src [N, F, h, w] (or [N, h, w]) -> the resampled logits [N, F, H, W] (or [N, H, W]) in float64, the taps evaluated in
    ``arith``.  ``src`` is taken as it is (round it to the dtype under test first)."""
    if src.dim() == 4:
        N, F = src.shape[:2]
        return resample(src.reshape(N * F, *src.shape[2:]), size, arith).reshape(N, F, size[0], size[1])
    return resample(src, size, arith)


def probabilities(src, size, arith=torch.float32):
    """sigmoid of :func:`logits`, by the header's expression."""
    x = logits(src, size, arith)
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def terms(a, b, size, arith=torch.float32):
    """(inter [F, Na, Nb], sum_a [F, Na], sum_b [F, Nb]) in float64; a, b [N, F, h, w]."""
    pa, pb = probabilities(a, size, arith).flatten(2), probabilities(b, size, arith).flatten(2)
    return torch.einsum("ifk,jfk->fij", pa, pb), pa.sum(2).t(), pb.sum(2).t()


def soft_iou(a, b, size, reduce="volume", eps=1e-6, arith=torch.float32):
    """[Na, Nb] in float64; a, b [N, F, h, w] or [N, h, w]."""
    if a.dim() == 3:
        a, b = a[:, None], b[:, None]
    inter, sa, sb = terms(a, b, size, arith)
    if reduce == "frame":
        return (inter / (sa[:, :, None] + sb[:, None, :] - inter).clamp(min=eps)).mean(0)
    I, Sa, Sb = inter.sum(0), sa.sum(0), sb.sum(0)
    return I / (Sa[:, None] + Sb[None, :] - I).clamp(min=eps)


def binarize(src, size, arith=torch.float32):
    """(bits [N, H, W] bool: x > 0; the resampled logits x in float64)."""
    x = logits(src, size, arith)
    return x > 0, x


def blob_logits(n, f, h, w, seed, gain=25.0, dtype=F64):
    """Smooth blob fields times a gain: [n, f, h, w] logits whose masks are compact regions of differing place and size, so
    that IoUs between them spread from near 0 to near 1 (pure noise gives 0.30 to 0.37 everywhere)."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.linspace(0, 1, h, dtype=F64).view(1, 1, h, 1)
    xs = torch.linspace(0, 1, w, dtype=F64).view(1, 1, 1, w)
    cy, cx = torch.rand(n, 1, 1, 1, generator=g, dtype=F64), torch.rand(n, 1, 1, 1, generator=g, dtype=F64)
    drift = 0.05 * torch.randn(n, f, 1, 1, generator=g, dtype=F64)
    rad = 0.15 + 0.35 * torch.rand(n, 1, 1, 1, generator=g, dtype=F64)
    d2 = (ys - cy - drift) ** 2 + (xs - cx + drift) ** 2
    field = 1.0 - 2.0 * d2 / rad ** 2 + 0.1 * torch.randn(n, f, h, w, generator=g, dtype=F64)
    return (gain * field).to(dtype)


# ---- the binarise cases the CPU and the GPU tests share ------------------------------------------------------------------
# (the last one is downsampled so steeply that a workgroup's source rows do not fit its LDS stage: it reads memory)
BINARIZE_CASES = [((12, 20), (45, 80)), ((7, 9), (27, 35)), ((26, 22), (13, 11)), ((13, 17), (13, 17)), ((200, 64), (5, 8))]
BINARIZE_CAP = 1e-3         # the largest share of pixels a comparison of bits may leave out


def binarize_case(index, dtype=torch.float32, n=3):
    """(src [n, h, w] random logits of gain 2.5 rounded to ``dtype``, the target size) of case ``index``."""
    (h, w), size = BINARIZE_CASES[index]
    g = torch.Generator().manual_seed(300 + index)
    return (2.5 * torch.randn(n, h, w, generator=g)).to(dtype), size


def near_zero(x, src):
    """The pixels a comparison of bits leaves out: |x| < 1e-5 * max|src|, far above the float32 rounding of the four
    products and three sums of x (a few 1e-7 * max|src|), so that outside them the sign of x is the oracle's."""
    return x.abs() < 1e-5 * float(src.abs().max())

"""Host side of the modulated deformable convolution (include/mdcn.h): argument checks, the
channels-last copy of the input, the batch-chunk loop under the workspace bound, and the GEMMs with the weights
(``torch`` -> rocBLAS) around the two HIP kernels.  The custom ops of :mod:`devis_amd.ops` run exactly this code.

``grad_input`` is by default a sum of float atomics, whose last bits depend on the order the adds arrive in.
:class:`reproducible_grad_input` opts in to the order-independent fixed-point sum of include/mdcn.h
(``mdcn_backward_input_fixed``): bitwise the same from run to run, for an image alone or in a batch, under any chunking.
That mode holds one more buffer of 8 + 1/2 bytes per element of the chunk's ``grad_input`` (int64 accumulators and class
nibbles); the other gradients are computed exactly as without it.

There is no CPU path and no eager fallback: CPU tensors raise, a failing kernel call raises.
"""
import warnings

import torch

from .. import _mdcn
from ._common import _check_device, _require

# Bound on ONE column buffer ([chunk * Ho * Wo, Kh * Kw * C] in the input's dtype).  A call is cut into chunks of whole images
# so that the buffer stays under it (one image is the smallest chunk, whatever its size); the forward holds one such
# buffer, a backward that computes grad_weight two (columns and grad_columns).  A constant, never derived from free memory:
# the chunking -- and with it the order of grad_weight's sum over chunks -- is the same on every run.
# (With reproducible_grad_input a backward also holds the fixed-point workspace of one chunk, 8 + 1/2 bytes per element of
# the chunk's grad_input; the chunk size is still chosen from the column bound alone.)
WORKSPACE_BYTES = 256 << 20

# which gradients a backward computes (the `grads` argument of the backward op)
NEED_INPUT, NEED_OFFSET, NEED_MASK, NEED_WEIGHT, NEED_BIAS = 1, 2, 4, 8, 16
NEED_ALL = 31
# Beside the NEED_* bits the `grads` argument may carry what a caller pinned for this call (the module's
# ``reproducible_grad_input`` attribute, the operator's keyword): grad_input by the fixed-point sum / by float atomics,
# whatever the process-wide switch says.  Neither bit set: the switch decides, when the backward runs.
PIN_FIXED, PIN_FLOAT = 32, 64
PIN_BITS = PIN_FIXED | PIN_FLOAT

_reproducible = False


class reproducible_grad_input:
    """Opt in to (or, with ``enabled=False``, out of) the order-independent ``grad_input`` of ``deform_conv2d``.

    A plain call ``reproducible_grad_input()`` sets the process-wide default; ``with reproducible_grad_input():`` restores
    the previous value on exit, and nests.  The switch is read when a backward RUNS, as
    ``torch.use_deterministic_algorithms`` is: the ``with`` block has to span the backward pass.  With it on, a backward
    that needs ``grad_input`` does not raise or warn under ``torch.use_deterministic_algorithms(True)``, and ``grad_input``
    comes from the fixed-point path whether or not that flag is set."""

    def __init__(self, enabled=True):
        global _reproducible
        self.previous = _reproducible
        _reproducible = bool(enabled)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _reproducible
        _reproducible = self.previous
        return False


def reproducible_grad_input_enabled():
    """The process-wide switch of :class:`reproducible_grad_input`."""
    return _reproducible


def pin_bits(pinned):
    """None / True / False (what a caller pinned for one call) -> the PIN_* bits of the backward's `grads`."""
    return 0 if pinned is None else (PIN_FIXED if pinned else PIN_FLOAT)


def input_mode(grads):
    """`grads` -> (its NEED_* bits, whether grad_input comes from the fixed-point path): what was pinned for the call,
    else the process-wide switch as it stands now."""
    pinned = grads & PIN_BITS
    _require(pinned != PIN_BITS, "grads pins grad_input to both of its paths")
    need = grads & NEED_ALL
    fixed = bool(need & NEED_INPUT) and (pinned == PIN_FIXED or (not pinned and _reproducible))
    return need, fixed


def _pair(v, name):
    if isinstance(v, (tuple, list)):
        _require(len(v) == 2, "%s must be an int or a pair" % name)
        return int(v[0]), int(v[1])
    return int(v), int(v)


def grads_mask(need_input, need_offset, need_mask, need_weight, need_bias):
    """``ctx.needs_input_grad`` flags -> the `grads` mask of the backward op."""
    return ((NEED_INPUT if need_input else 0) | (NEED_OFFSET if need_offset else 0) | (NEED_MASK if need_mask else 0) |
            (NEED_WEIGHT if need_weight else 0) | (NEED_BIAS if need_bias else 0))


def output_size(size, kernel, stride, padding, dilation):
    return (size + 2 * padding - dilation * (kernel - 1) - 1) // stride + 1


def check_shapes(input, offset, weight, bias, stride, padding, dilation, mask):
    """Shape and dtype contract of deform_conv2d (torchvision's); raises before anything is launched.  Works on fake
    tensors.  Returns (Ho, Wo, G)."""
    _require(input.dim() == 4 and offset.dim() == 4 and weight.dim() == 4, "input, offset and weight must be 4-D")
    N, C, H, W = input.shape
    Co, Cw, Kh, Kw = weight.shape
    if Cw != C:
        if Cw > 0 and C % Cw == 0:
            raise NotImplementedError("deform_conv2d: weight groups are not implemented (weight.shape[1] = %d, input has %d "
                                      "channels); only one weight group (weight.shape[1] == in_channels) is" % (Cw, C))
        raise RuntimeError("deform_conv2d: weight.shape[1] = %d does not match the input's %d channels" % (Cw, C))
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    _require(sh > 0 and sw > 0 and dh > 0 and dw > 0 and ph >= 0 and pw >= 0,
             "deform_conv2d: stride and dilation must be positive, padding not negative")
    _require(Kh > 0 and Kw > 0 and Co > 0 and C > 0, "deform_conv2d: weight must not be empty")
    Ho, Wo = output_size(H, Kh, sh, ph, dh), output_size(W, Kw, sw, pw, dw)
    _require(Ho > 0 and Wo > 0, "deform_conv2d: the output would be empty (%s x %s)" % (Ho, Wo))
    K = Kh * Kw
    _require(offset.shape[0] == N and offset.shape[2] == Ho and offset.shape[3] == Wo,
             "deform_conv2d: offset must be [N, 2*G*Kh*Kw, Ho, Wo] = [%s, 2*G*%d, %s, %s], got %s"
             % (N, K, Ho, Wo, tuple(offset.shape)))
    _require(offset.shape[1] > 0 and offset.shape[1] % (2 * K) == 0,
             "deform_conv2d: offset.shape[1] = %s is not a multiple of 2*Kh*Kw = %d" % (offset.shape[1], 2 * K))
    G = offset.shape[1] // (2 * K)
    _require(C % G == 0, "deform_conv2d: %d input channels are not a multiple of the %d offset groups" % (C, G))
    if mask is not None:
        _require(mask.dim() == 4 and mask.shape[0] == N and mask.shape[1] == G * K and mask.shape[2] == Ho and mask.shape[3] == Wo,
                 "deform_conv2d: mask must be [N, G*Kh*Kw, Ho, Wo] = [%s, %d, %s, %s], got %s"
                 % (N, G * K, Ho, Wo, tuple(mask.shape)))
        _require(mask.dtype == offset.dtype, "deform_conv2d: mask must have offset's dtype")
    if bias is not None:
        _require(bias.dim() == 1 and bias.shape[0] == Co, "deform_conv2d: bias must be [%d]" % Co)
        _require(bias.dtype == input.dtype, "deform_conv2d: bias must have input's dtype")
    _require(weight.dtype == input.dtype, "deform_conv2d: weight must have input's dtype")
    _mdcn.type_code(input.dtype, offset.dtype)      # raises on an unsupported pair
    return Ho, Wo, G


def alert_nondeterministic(grads):
    """grad_input is a sum of float atomics, so it depends on the order the adds arrive in: under
    ``torch.use_deterministic_algorithms(True)`` asking for it raises (warns with ``warn_only=True``), as PyTorch's own
    non-deterministic operators do.  The other four gradients are reproducible bit for bit.  (Not called when
    grad_input comes from the fixed-point path: see :func:`input_mode`.)"""
    if grads & NEED_INPUT and torch.are_deterministic_algorithms_enabled():
        msg = ("devis_amd::deform_conv2d_backward does not have a deterministic implementation of grad_input, but you set "
               "'torch.use_deterministic_algorithms(True%s)'. You can turn off determinism just for this operation, or detach "
               "the input (the other gradients are deterministic). An order-independent grad_input is opt-in: "
               "devis_amd.reproducible_grad_input(), or reproducible_grad_input=True on the ModulatedDeformableConv2d layer.")
        if torch.is_deterministic_algorithms_warn_only_enabled():
            warnings.warn(msg % ", warn_only=True", UserWarning, stacklevel=2)
        else:
            raise RuntimeError(msg % "")


def chunk_images(code, shape, N, workspace_bytes=None):
    """Images per chunk: as many as keep one column buffer within the bound, at least one."""
    bound = WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes
    per_image = _mdcn.workspace_bytes(code, shape, 1)
    return max(1, min(N, bound // max(per_image, 1)))


def _prepare(input, offset, weight, bias, stride, padding, dilation, mask):
    _check_device("deform_conv2d", [("input", input), ("offset", offset), ("weight", weight), ("bias", bias), ("mask", mask)])
    Ho, Wo, G = check_shapes(input, offset, weight, bias, stride, padding, dilation, mask)
    N, C, H, W = input.shape
    Co, _, Kh, Kw = weight.shape
    shape = _mdcn.Shape(N, C, H, W, Ho, Wo, Kh, Kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], G)
    code = _mdcn.type_code(input.dtype, offset.dtype)
    x = input.permute(0, 2, 3, 1).contiguous()                  # channels-last: a tap's corners are contiguous channel rows
    w2 = weight.permute(0, 2, 3, 1).reshape(Co, Kh * Kw * C)    # [Co, (k, c)]: the columns' order
    return shape, code, x, offset.contiguous(), None if mask is None else mask.contiguous(), w2


def _forward(input, offset, weight, bias, stride, padding, dilation, mask):
    """out [N, Co, Ho, Wo] = columns @ weight^T (+ bias), one batched GEMM per chunk written straight into NCHW: each
    image is the same GEMM whatever the chunking, so `out` does not depend on the workspace bound."""
    shape, code, x, offset, mask, w2 = _prepare(input, offset, weight, bias, stride, padding, dilation, mask)
    N, Co, P, KC = shape.N, weight.shape[0], shape.Ho * shape.Wo, w2.shape[1]
    out = torch.empty((N, Co, shape.Ho, shape.Wo), dtype=input.dtype, device=input.device)
    if N == 0:
        return out
    step = chunk_images(code, shape, N)
    cols = torch.empty((step * P, KC), dtype=input.dtype, device=input.device)
    for n0 in range(0, N, step):
        nb = min(step, N - n0)
        shape.N = nb
        _mdcn.im2col(code, x[n0:n0 + nb], offset[n0:n0 + nb], None if mask is None else mask[n0:n0 + nb], shape, cols)
        colsT = cols[:nb * P].view(nb, P, KC).transpose(1, 2)
        dst = out[n0:n0 + nb].view(nb, Co, P)
        if bias is None:
            torch.bmm(w2.expand(nb, Co, KC), colsT, out=dst)
        else:
            torch.baddbmm(bias.view(1, Co, 1).expand(nb, Co, P), w2.expand(nb, Co, KC), colsT, out=dst)
    return out


def _backward(grad_out, input, offset, weight, mask, stride, padding, dilation, grads=NEED_ALL):
    """(grad_input, grad_offset, grad_mask, grad_weight, grad_bias) for the gradients in ``grads``; the others are
    neither allocated nor computed and come back None (grad_mask also without a mask).  ``grads`` may carry a PIN_* bit;
    grad_input then, or with :class:`reproducible_grad_input` on, is the fixed-point sum of ``mdcn_backward_input_fixed``:
    chunks are whole images and its quanta are per image, so the chunking does not show in it (given the same
    grad_columns: a row of that GEMM is a sum over Co alone, and rocBLAS gave it the same bits for every chunk size
    tests/test_dcn_reproducible_gpu.py tries; the library's own guarantee starts at grad_columns)."""
    grads, fixed = input_mode(grads)
    if not fixed:
        alert_nondeterministic(grads)
    _check_device("deform_conv2d", [("input", input), ("grad_out", grad_out)])
    shape, code, x, offset, mask, w2 = _prepare(input, offset, weight, None, stride, padding, dilation, mask)
    N, C, H, W = input.shape
    Co, _, Kh, Kw = weight.shape
    P, KC = shape.Ho * shape.Wo, w2.shape[1]
    _require(tuple(grad_out.shape) == (N, Co, shape.Ho, shape.Wo) and grad_out.dtype == input.dtype,
             "deform_conv2d: grad_out must be [N, Co, Ho, Wo] in input's dtype")
    dev, dt = input.device, input.dtype
    acc = torch.float64 if dt == torch.float64 else torch.float32
    want_in = bool(grads & NEED_INPUT)
    want_s = bool(grads & NEED_OFFSET) or (bool(grads & NEED_MASK) and mask is not None)
    want_w, want_b = bool(grads & NEED_WEIGHT), bool(grads & NEED_BIAS)
    kernel_grads = (_mdcn.GRAD_INPUT if want_in and not fixed else 0) | (_mdcn.GRAD_SAMPLING if want_s else 0)

    gin_acc = None
    if want_in:     # the float atomics add into zeros; the fixed-point path writes every element
        gin_acc = (torch.empty if fixed else torch.zeros)((N, H, W, C), dtype=acc, device=dev)
    goff = torch.empty_like(offset) if want_s else None
    gmsk = torch.empty_like(mask) if want_s and mask is not None else None
    gw_acc = torch.zeros((Co, KC), dtype=acc, device=dev) if want_w else None
    if N > 0 and (kernel_grads or fixed or want_w):
        step = chunk_images(code, shape, N)
        gcols = torch.empty((step * P, KC), dtype=dt, device=dev) if kernel_grads or fixed else None
        fixed_ws = torch.empty(_mdcn.fixed_workspace_bytes(code, shape, step), dtype=torch.uint8, device=dev) if fixed else None
        cols = torch.empty((step * P, KC), dtype=dt, device=dev) if want_w else None
        for n0 in range(0, N, step):
            nb = min(step, N - n0)
            shape.N = nb
            sl = slice(n0, n0 + nb)
            go = grad_out[sl].permute(0, 2, 3, 1).reshape(nb * P, Co)      # [pixels, Co] (a copy unless channels-last)
            mk = None if mask is None else mask[sl]
            if kernel_grads or fixed:
                torch.mm(go, w2, out=gcols[:nb * P])
            if kernel_grads:
                _mdcn.backward(kernel_grads, code, x[sl], offset[sl], mk, gcols, shape,
                               gin_acc[sl] if kernel_grads & _mdcn.GRAD_INPUT else None, None if goff is None else goff[sl],
                               None if gmsk is None else gmsk[sl])
            if fixed:
                _mdcn.backward_input_fixed(code, offset[sl], mk, gcols, shape, fixed_ws, gin_acc[sl])
            if want_w:
                _mdcn.im2col(code, x[sl], offset[sl], mk, shape, cols)
                part = torch.mm(go.t(), cols[:nb * P])
                gw_acc += part if part.dtype == acc else part.to(acc)
    grad_input = grad_weight = grad_bias = None
    if want_in:     # one rounding to the storage type, on the way back to NCHW
        grad_input = torch.empty((N, C, H, W), dtype=dt, device=dev).copy_(gin_acc.permute(0, 3, 1, 2))
    if want_w:
        grad_weight = torch.empty_like(weight, memory_format=torch.contiguous_format).copy_(
            gw_acc.view(Co, Kh, Kw, C).permute(0, 3, 1, 2))
    if want_b:
        grad_bias = grad_out.sum(dim=(0, 2, 3), dtype=acc).to(dt)
    return (grad_input, goff if grads & NEED_OFFSET else None, gmsk if grads & NEED_MASK else None, grad_weight, grad_bias)


def setup_context(ctx, inputs, output):
    # inputs: the 8 of ``deform_conv2d``, or the 9 of ``deform_conv2d_pinned`` (reproducible_grad_input last).
    # ctx.pinned exists only in the second case: backward() tells the two ops apart by it.
    input, offset, weight, bias, stride, padding, dilation, mask = inputs[:8]
    ctx.geometry = (stride, padding, dilation)
    if len(inputs) > 8:
        ctx.pinned = bool(inputs[8])
    ctx.save_for_backward(input, offset, weight, mask)


def backward(run, ctx, grad_out):
    """The autograd formula of both forward ops; ``run`` has the signature of :func:`_backward`: the backward op with its
    empty gradients mapped to None.  One gradient slot per input the op was given."""
    input, offset, weight, mask = ctx.saved_tensors
    needs = ctx.needs_input_grad
    pinned = getattr(ctx, "pinned", None)
    grads = grads_mask(needs[0], needs[1], needs[7] and mask is not None, needs[2], needs[3]) | pin_bits(pinned)
    gi, go, gm, gw, gb = run(grad_out, input, offset, weight, mask, *ctx.geometry, grads)
    slots = (gi, go, gw, gb, None, None, None, gm)
    return slots if pinned is None else slots + (None,)

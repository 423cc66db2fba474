"""Host side of the encoder's input projections (include/inputproj.h):
``group_norm_tokens(xs, num_groups, weights, biases)`` = the ``GroupNorm`` of the reference's ``input_proj[l]`` of every pyramid
level written once, channels last, at the level's token offset -- ``DeformableTransformer.prepare_data``'s ``src_flatten``
without the normalised NCHW maps, their transposed views and the ``cat``.  Argument checks, the output and workspace tensors,
the kernel launches and the autograd Function over the ``3 L`` tensors.

Every sum has a fixed order and there are no atomics: every result is bitwise reproducible and nothing here raises or warns
under ``torch.use_deterministic_algorithms(True)``.

As :mod:`devis_amd.functions.swin_ends`'s, this is not a ``torch.library`` op: the public function computes the TORCH COMPOSITE
-- the reference's chain of ``F.group_norm``, ``flatten``, ``transpose`` and ``cat`` -- while
``torch.compiler.is_compiling()``, on CPU tensors, in float64 or another dtype mix the kernels do not take, above the kernels'
limits and without elements.  On the kernel route a failing call raises.
"""
import torch
import torch.nn.functional as F

from .. import _inputproj
from ._common import _check_device, _require

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
HALVES = (torch.bfloat16, torch.float16)
OP = "group_norm_tokens"


def supported(x_dtype, param_dtype, y_dtype):
    """Whether the kernels take this combination of dtypes (include/inputproj.h)."""
    if x_dtype not in DTYPES or param_dtype not in DTYPES or y_dtype not in DTYPES:
        return False
    if x_dtype == torch.float32:
        return param_dtype == torch.float32
    return param_dtype in (x_dtype, torch.float32) and y_dtype in (x_dtype, torch.float32)


def _check(xs, num_groups, weights, biases):
    xs, weights, biases = list(xs), list(weights), list(biases)
    _require(len(xs) >= 1 and len(weights) == len(xs) and len(biases) == len(xs),
             "%s: one weight and one bias per map, got %d maps, %d weights and %d biases" % (OP, len(xs), len(weights), len(biases)))
    first = xs[0]
    _require(first.dim() == 4, "%s: a map must be [N, C, H, W], got %s" % (OP, tuple(first.shape)))
    N, C = first.shape[:2]
    _require(isinstance(num_groups, int) and num_groups >= 1 and C % num_groups == 0,
             "%s: the %d channels must be a multiple of num_groups = %s >= 1" % (OP, C, num_groups))
    for l, (x, w, b) in enumerate(zip(xs, weights, biases)):
        _require(x.dim() == 4 and tuple(x.shape[:2]) == (N, C) and x.dtype == first.dtype and x.device == first.device,
                 "%s: map %d must be [%d, %d, H, W] in the dtype and on the device of map 0, got %s %s" % (OP, l, N, C, tuple(x.shape), x.dtype))
        for name, t in (("weight", w), ("bias", b)):
            _require(t is not None and tuple(t.shape) == (C,) and t.dtype == weights[0].dtype and t.device == first.device,
                     "%s: %s %d must be [%d] in the dtype of weight 0 and on the maps' device" % (OP, name, l, C))
    return xs, weights, biases


def _shape(xs, num_groups):
    return _inputproj.shape_of(xs[0].shape[0], xs[0].shape[1], num_groups, [tuple(x.shape[2:]) for x in xs])


def _forward(xs, weights, biases, num_groups, eps, out_dtype):
    """(tokens [N, S, C], mean [N, L, G], rstd [N, L, G]): the statistics launch, its combine launch when a group spans several
    chunks, and the apply launch.  A map that is not dense NCHW -- a channels-last one -- is made dense first."""
    _check_device(OP, [("x%d" % l, x) for l, x in enumerate(xs)] + [("weight%d" % l, w) for l, w in enumerate(weights)] +
                  [("bias%d" % l, b) for l, b in enumerate(biases)])
    first = xs[0]
    N, C = first.shape[:2]
    shape = _shape(xs, num_groups)
    y_dtype = first.dtype if out_dtype is None else out_dtype
    tokens = torch.empty((N, sum(x.shape[2] * x.shape[3] for x in xs), C), dtype=y_dtype, device=first.device)
    mean = torch.empty((N, len(xs), num_groups), dtype=torch.float32, device=first.device)
    rstd = torch.empty_like(mean)
    nbytes = _inputproj.forward_workspace_bytes(shape)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=first.device) if nbytes else None
    _inputproj.forward(_inputproj.types_of(first.dtype, weights[0].dtype, y_dtype), [x.contiguous() for x in xs],
                       [w.contiguous() for w in weights], [b.contiguous() for b in biases], eps, shape, workspace, tokens, mean, rstd)
    return tokens, mean, rstd


def _backward(grad_tokens, xs, weights, mean, rstd, num_groups, wants):
    """``(grad_xs, grad_weights, grad_biases)``, three lists with None where ``wants`` -- three lists of bools -- is False: the
    sums launch, its combine launch, and the grad_x launch when a map's gradient is asked for."""
    _check_device(OP, [("grad_tokens", grad_tokens), ("mean", mean), ("rstd", rstd)] + [("x%d" % l, x) for l, x in enumerate(xs)] +
                  [("weight%d" % l, w) for l, w in enumerate(weights)])
    want_x, want_w, want_b = wants
    shape = _shape(xs, num_groups)
    _require(tuple(grad_tokens.shape) == (xs[0].shape[0], sum(x.shape[2] * x.shape[3] for x in xs), xs[0].shape[1]),
             "%s: the gradient of the tokens must have their shape" % OP)
    dense = [x.contiguous() for x in xs]
    grad_xs = [torch.empty(x.shape, dtype=x.dtype, device=x.device) if want else None for x, want in zip(xs, want_x)]
    grad_ws = [torch.empty_like(w) if want else None for w, want in zip(weights, want_w)]
    grad_bs = [torch.empty_like(w) if want else None for w, want in zip(weights, want_b)]
    workspace = torch.empty(_inputproj.backward_workspace_bytes(shape), dtype=torch.uint8, device=grad_tokens.device)
    _inputproj.backward(_inputproj.types_of(xs[0].dtype, weights[0].dtype, grad_tokens.dtype), dense,
                        [w.contiguous() for w in weights], mean.contiguous(), rstd.contiguous(), grad_tokens.contiguous(), shape,
                        workspace, grad_xs, grad_ws, grad_bs)
    return grad_xs, grad_ws, grad_bs


class GroupNormTokensFunction(torch.autograd.Function):
    """``group_norm_tokens`` for eager code: ``apply(num_groups, eps, out_dtype, *xs, *weights, *biases)`` -> (tokens, mean, rstd).
    Saves the maps, the weights, mean and rstd -- never the tokens.  The backward computes the gradients autograd asks for and
    launches nothing when it asks for none."""
    @staticmethod
    def forward(num_groups, eps, out_dtype, *tensors):
        L = len(tensors) // 3
        return _forward(tensors[:L], tensors[L:2 * L], tensors[2 * L:], num_groups, eps, out_dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        num_groups, eps, out_dtype = inputs[:3]
        tensors = inputs[3:]
        L = len(tensors) // 3
        tokens, mean, rstd = output
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mean, rstd)
        ctx.num_groups, ctx.levels = num_groups, L
        ctx.save_for_backward(*tensors[:2 * L], mean, rstd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_tokens, grad_mean, grad_rstd):
        L = ctx.levels
        needs = ctx.needs_input_grad[3:]
        wants = (list(needs[:L]), list(needs[L:2 * L]), list(needs[2 * L:]))
        if grad_tokens is None or not any(any(w) for w in wants):
            return (None,) * (3 + 3 * L)
        saved = ctx.saved_tensors
        xs, weights, mean, rstd = saved[:L], saved[L:2 * L], saved[2 * L], saved[2 * L + 1]
        grad_xs, grad_ws, grad_bs = _backward(grad_tokens, xs, weights, mean, rstd, ctx.num_groups, wants)
        return (None, None, None) + tuple(grad_xs) + tuple(grad_ws) + tuple(grad_bs)


def group_norm_tokens_composite(xs, num_groups, weights, biases, eps=1e-5, out_dtype=None):
    """What :func:`group_norm_tokens` computes, by torch: the reference's ``GroupNorm`` of every level, ``flatten(2)``,
    ``transpose(1, 2)`` and ``cat`` over the levels."""
    tokens = torch.cat([F.group_norm(x, num_groups, w, b, eps).flatten(2).transpose(1, 2) for x, w, b in zip(xs, weights, biases)], 1)
    return tokens if out_dtype is None else tokens.to(out_dtype)


def takes_kernels(xs, num_groups, weights, out_dtype=None):
    """Whether a call goes to the kernels: not while compiling, not on the CPU, not without elements, at most
    ``INPUTPROJ_MAX_LEVELS`` levels and ``INPUTPROJ_MAX_CHANNELS`` channels, and a dtype mix of include/inputproj.h."""
    first = xs[0]
    if torch.compiler.is_compiling() or not first.is_cuda or any(x.numel() == 0 for x in xs):
        return False
    if not (len(xs) <= _inputproj.MAX_LEVELS and first.shape[1] <= _inputproj.MAX_CHANNELS):
        return False
    return supported(first.dtype, weights[0].dtype, first.dtype if out_dtype is None else out_dtype)


def group_norm_tokens(xs, num_groups, weights, biases, eps=1e-5, out_dtype=None):
    """The GroupNorms of the reference's input projections and ``prepare_data``'s flattening as HIP kernel passes
    (include/inputproj.h): ``xs`` a sequence of ``L`` maps ``[N, C, H_l, W_l]`` -- the convolutions' outputs --, ``weights`` and
    ``biases`` sequences of ``[C]`` -> ``tokens [N, sum(H_l * W_l), C]``, exactly what
    ``cat([GroupNorm_l(x_l).flatten(2).transpose(1, 2)], 1)`` returns.  No normalised NCHW map exists, forward or backward.

    ``C % num_groups == 0``, ``C <= 1024``, ``L <= 8``.  dtypes: maps in float32, bfloat16 or float16, parameters in the maps'
    dtype or float32, ``out_dtype`` (default: the maps') the maps' dtype or float32 -- float32 tokens from 16-bit maps with
    float32 parameters are what stock GroupNorm returns under autocast -- or 16-bit beside float32 maps.  Arithmetic is float32
    (the variance by a shifted two-sweep sum per chunk and Chan's combination, never ``E[x^2] - E[x]^2``); the tokens are
    rounded once.  Differentiable once in every map, weight and bias; the backward keeps the maps, ``mean`` and ``rstd``, never
    the tokens, and computes only what autograd asks for.  A map that is not dense NCHW is made dense on the host.  On the CPU,
    in float64 or another dtype mix, above the limits, without elements and while ``torch.compiler.is_compiling()`` this is the
    torch composite."""
    xs, weights, biases = _check(xs, num_groups, weights, biases)
    if not takes_kernels(xs, num_groups, weights, out_dtype):
        return group_norm_tokens_composite(xs, num_groups, weights, biases, eps, out_dtype)
    if torch.is_grad_enabled() and any(t.requires_grad for t in xs + weights + biases):
        return GroupNormTokensFunction.apply(num_groups, eps, out_dtype, *xs, *weights, *biases)[0]
    return _forward([x.detach() for x in xs], weights, biases, num_groups, eps, out_dtype)[0]

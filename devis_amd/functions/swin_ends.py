"""Host side of the two ends of the Swin backbone (include/swinends.h):
``patch_embed_norm(image, proj_weight, proj_bias, norm_weight, norm_bias)`` = the reference's ``PatchEmbed`` -- zero padding,
``p x p`` / stride-``p`` projection, LayerNorm -- written once, in token order, and ``layer_norm_to_map(x, H, W, weight, bias)`` =
a stage's output norm written once, as the NCHW map.  Argument checks, the output and workspace tensors, the kernel launches and
the two autograd Functions.

Every sum has a fixed order and there are no atomics: every result is bitwise reproducible and nothing here raises or warns
under ``torch.use_deterministic_algorithms(True)``.

As :mod:`devis_amd.functions.pre_norm`'s, these two are not ``torch.library`` ops: the public functions compute the TORCH
COMPOSITE -- the reference's chain of ``F.pad``, ``F.conv2d``, ``F.layer_norm``, ``permute`` and ``contiguous`` -- while
``torch.compiler.is_compiling()``, on CPU tensors, in float64 or another dtype mix the kernels do not take, above the kernels'
limits, and (the embedding) when the image requires a gradient.  On the kernel route a failing call raises.
"""
import torch
import torch.nn.functional as F

from .. import _swinends
from ._common import _check_device, _require

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
HALVES = (torch.bfloat16, torch.float16)


def _on_gpu(t):
    return t.is_cuda


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _new(like, on):
    return torch.empty(like.shape, dtype=like.dtype, device=like.device) if on else None


def _dense(t):
    return None if t is None else t.contiguous()


# ---- patch_embed_norm -------------------------------------------------------------------------------------------------------

def embed_supported(image_dtype, param_dtype, y_dtype):
    """Whether the embedding kernels take this combination of dtypes (include/swinends.h)."""
    if image_dtype not in DTYPES or param_dtype not in DTYPES or y_dtype not in DTYPES:
        return False
    return image_dtype == param_dtype and (y_dtype == image_dtype or (image_dtype == torch.float32 and y_dtype in HALVES))


def _embed_check(image, proj_weight, proj_bias, norm_weight, norm_bias):
    op = "patch_embed_norm"
    _require(image.dim() == 4, "%s: image must be [B, Cin, H, W], got %s" % (op, tuple(image.shape)))
    _require(proj_weight.dim() == 4 and proj_weight.shape[1] == image.shape[1] and proj_weight.shape[2] == proj_weight.shape[3]
             and proj_weight.shape[2] >= 1,
             "%s: proj_weight must be [C, Cin = %d, p, p], got %s" % (op, image.shape[1], tuple(proj_weight.shape)))
    C = proj_weight.shape[0]
    _require((norm_weight is None) == (norm_bias is None), "%s: norm_weight and norm_bias are given together or not at all" % op)
    for name, t in (("proj_bias", proj_bias), ("norm_weight", norm_weight), ("norm_bias", norm_bias)):
        _require(t is None or (tuple(t.shape) == (C,) and t.dtype == proj_weight.dtype),
                 "%s: %s must be [%d] in proj_weight's dtype" % (op, name, C))


def _embed_shape(image, proj_weight):
    B, Cin, H, W = image.shape
    return _swinends.EmbedShape(B, Cin, H, W, proj_weight.shape[2], proj_weight.shape[0])


def _embed_forward(image, proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype, want_stats=True):
    """(tokens [B, Hp * Wp, C], mean, rstd); the float32 statistics are None without a norm or unless ``want_stats``."""
    op = "patch_embed_norm"
    _check_device(op, [("image", image), ("proj_weight", proj_weight), ("proj_bias", proj_bias), ("norm_weight", norm_weight),
                       ("norm_bias", norm_bias)])
    B, Cin, H, W = image.shape
    C, p = proj_weight.shape[0], proj_weight.shape[2]
    L = (-(-H // p)) * (-(-W // p))
    y_dtype = image.dtype if out_dtype is None else out_dtype
    tokens = torch.empty((B, L, C), dtype=y_dtype, device=image.device)
    stats = want_stats and norm_weight is not None
    mean = torch.empty((B, L), dtype=torch.float32, device=image.device) if stats else None
    rstd = torch.empty((B, L), dtype=torch.float32, device=image.device) if stats else None
    _swinends.embed_forward(_swinends.embed_types_of(image.dtype, proj_weight.dtype, y_dtype), image.contiguous(),
                            proj_weight.contiguous(), _dense(proj_bias), _dense(norm_weight), _dense(norm_bias), eps,
                            _embed_shape(image, proj_weight), tokens, mean, rstd)
    return tokens, mean, rstd


def _embed_backward(grad_tokens, image, proj_weight, proj_bias, norm_weight, mean, rstd, wants):
    """(grad_proj_weight, grad_proj_bias, grad_norm_weight, grad_norm_bias), None where ``wants`` is False: two launches."""
    op = "patch_embed_norm"
    want_pw, want_pb, want_nw, want_nb = wants
    _check_device(op, [("grad_tokens", grad_tokens), ("image", image), ("proj_weight", proj_weight), ("proj_bias", proj_bias),
                       ("norm_weight", norm_weight), ("mean", mean), ("rstd", rstd)])
    shape = _embed_shape(image, proj_weight)
    grad_pw = _new(proj_weight, want_pw)
    grad_pb = torch.empty(proj_weight.shape[:1], dtype=proj_weight.dtype, device=proj_weight.device) if want_pb else None
    grad_nw, grad_nb = (_new(norm_weight, want) if norm_weight is not None else None for want in (want_nw, want_nb))
    workspace = torch.empty(_swinends.embed_workspace_bytes(shape, want_pw), dtype=torch.uint8, device=image.device)
    _swinends.embed_backward(_swinends.embed_types_of(image.dtype, proj_weight.dtype, grad_tokens.dtype), image.contiguous(),
                             proj_weight.contiguous(), _dense(proj_bias), _dense(norm_weight), _dense(mean), _dense(rstd),
                             grad_tokens.contiguous(), shape, workspace, grad_pw, grad_pb, grad_nw, grad_nb)
    return grad_pw, grad_pb, grad_nw, grad_nb


class PatchEmbedNormFunction(torch.autograd.Function):
    """``patch_embed_norm`` for eager code: ``apply(image, proj_weight, proj_bias or None, norm_weight or None, norm_bias or None,
    eps, out_dtype)`` -> (tokens, mean, rstd).  Saves the image, the parameters, mean and rstd -- nothing of the tokens' size: the
    backward projects the image again.  The image gets no gradient.  The backward computes the gradients autograd asks for and
    launches nothing when it asks for none."""
    @staticmethod
    def forward(image, proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype):
        return _embed_forward(image, proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        image, proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype = inputs
        tokens, mean, rstd = output
        ctx.set_materialize_grads(False)
        if mean is not None:
            ctx.mark_non_differentiable(mean, rstd)
        ctx.save_for_backward(image, proj_weight, proj_bias, norm_weight, mean, rstd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_tokens, grad_mean, grad_rstd):
        wants = tuple(ctx.needs_input_grad[1:5])
        if not any(wants) or grad_tokens is None:
            return (None,) * 7
        image, proj_weight, proj_bias, norm_weight, mean, rstd = ctx.saved_tensors
        return (None,) + _embed_backward(grad_tokens, image, proj_weight, proj_bias, norm_weight, mean, rstd, wants) + (None,) * 2


def patch_embed_norm_composite(image, proj_weight, proj_bias, norm_weight, norm_bias, eps=1e-5, out_dtype=None):
    """What :func:`patch_embed_norm` computes, by torch: the reference's ``PatchEmbed.forward`` up to the token tensor."""
    p = proj_weight.shape[2]
    H, W = image.shape[2:]
    if W % p or H % p:
        image = F.pad(image, (0, -W % p, 0, -H % p))
    tokens = F.conv2d(image, proj_weight, proj_bias, stride=p).flatten(2).transpose(1, 2)
    if norm_weight is not None:
        tokens = F.layer_norm(tokens, (tokens.shape[-1],), norm_weight, norm_bias, eps)
    else:
        tokens = tokens.contiguous()
    return tokens if out_dtype is None else tokens.to(out_dtype)


def embed_takes_kernels(image, proj_weight, out_dtype):
    """Whether a call goes to the kernels: not while compiling, not on the CPU, not without elements, not for a gradient of the
    image, within ``SWINENDS_MAX_PATCH`` and ``SWINENDS_MAX_EMBED`` and with a dtype mix of include/swinends.h."""
    if torch.compiler.is_compiling() or not _on_gpu(image) or image.numel() == 0:
        return False
    if torch.is_grad_enabled() and image.requires_grad:
        return False
    C, Cin, p = proj_weight.shape[:3]
    if not (1 <= C <= _swinends.MAX_EMBED and 1 <= Cin * p * p <= _swinends.MAX_PATCH):
        return False
    return embed_supported(image.dtype, proj_weight.dtype, image.dtype if out_dtype is None else out_dtype)


def patch_embed_norm(image, proj_weight, proj_bias, norm_weight, norm_bias, eps=1e-5, out_dtype=None):
    """The reference's ``PatchEmbed`` as one HIP kernel pass (include/swinends.h): ``image [B, Cin, H, W]``, ``proj_weight
    [C, Cin, p, p]``, ``proj_bias [C]`` or None, ``norm_weight`` / ``norm_bias`` ``[C]`` or both None (``patch_norm=False``) ->
    ``tokens [B, ceil(H / p) * ceil(W / p), C]``: the LayerNorm over ``C`` of the projected ``p x p`` patches, a pixel outside
    ``H x W`` counting as exactly 0.  No padded image, no NCHW convolution output and no transposed copy exists.

    ``Cin * p * p <= 192``, ``C <= 1024``.  dtypes: one of float32 / bfloat16 / float16 for all, or float32 image and parameters
    with a 16-bit ``out_dtype``.  Arithmetic is float32; the tokens are rounded once.  Differentiable in the four parameters
    (once); the backward keeps ``mean`` and ``rstd`` only and projects the image again.  When the image requires a gradient,
    on the CPU, in float64 or another dtype mix, above the limits and while ``torch.compiler.is_compiling()`` this is the torch
    composite."""
    _embed_check(image, proj_weight, proj_bias, norm_weight, norm_bias)
    if not embed_takes_kernels(image, proj_weight, out_dtype):
        return patch_embed_norm_composite(image, proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype)
    if _wants_grad(proj_weight, proj_bias, norm_weight, norm_bias):
        return PatchEmbedNormFunction.apply(image, proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype)[0]
    return _embed_forward(image.detach(), proj_weight, proj_bias, norm_weight, norm_bias, eps, out_dtype, want_stats=False)[0]


# ---- layer_norm_to_map ------------------------------------------------------------------------------------------------------

def map_supported(x_dtype, param_dtype, y_dtype):
    """Whether the output-norm kernels take this combination of dtypes (include/swinends.h)."""
    if x_dtype not in DTYPES or param_dtype not in DTYPES or y_dtype not in DTYPES:
        return False
    if x_dtype == torch.float32:
        return param_dtype == torch.float32
    return y_dtype == x_dtype and param_dtype in (x_dtype, torch.float32)


def _map_forward(x, weight, bias, H, W, eps, out_dtype, want_stats=True):
    """(y [B, C, H, W], mean, rstd) from x [B, H * W, C]."""
    op = "layer_norm_to_map"
    _check_device(op, [("x", x), ("weight", weight), ("bias", bias)])
    B, L, C = x.shape
    y_dtype = x.dtype if out_dtype is None else out_dtype
    y = torch.empty((B, C, H, W), dtype=y_dtype, device=x.device)
    mean = torch.empty((B, L), dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty((B, L), dtype=torch.float32, device=x.device) if want_stats else None
    _swinends.map_forward(_swinends.map_types_of(x.dtype, y_dtype, weight.dtype), x.contiguous(), weight.contiguous(),
                          bias.contiguous(), eps, _swinends.MapShape(B, H, W, C), y, mean, rstd)
    return y, mean, rstd


def _map_backward(grad_y, x, weight, mean, rstd, H, W, wants):
    """(grad_x [B, H * W, C], grad_weight, grad_bias), None where ``wants`` is False; a ``grad_y`` that is not dense NCHW -- a
    channels-last one -- is made dense first."""
    op = "layer_norm_to_map"
    want_x, want_w, want_b = wants
    _check_device(op, [("grad_y", grad_y), ("x", x), ("weight", weight), ("mean", mean), ("rstd", rstd)])
    B, L, C = x.shape
    _require(tuple(grad_y.shape) == (B, C, H, W), "%s: the gradient of y must have y's shape" % op)
    shape = _swinends.MapShape(B, H, W, C)
    grad_x, grad_weight, grad_bias = _new(x, want_x), _new(weight, want_w), _new(weight, want_b)
    workspace = None
    if want_w or want_b:
        workspace = torch.empty(_swinends.map_workspace_bytes(shape), dtype=torch.uint8, device=x.device)
    _swinends.map_backward(_swinends.map_types_of(x.dtype, grad_y.dtype, weight.dtype), x.contiguous(), weight.contiguous(),
                           mean.contiguous(), rstd.contiguous(), grad_y.contiguous(), shape, workspace, grad_x, grad_weight, grad_bias)
    return grad_x, grad_weight, grad_bias


class LayerNormToMapFunction(torch.autograd.Function):
    """``layer_norm_to_map`` for eager code: ``apply(x, weight, bias, H, W, eps, out_dtype)`` -> (y, mean, rstd).  Saves x, weight,
    mean and rstd -- never y."""
    @staticmethod
    def forward(x, weight, bias, H, W, eps, out_dtype):
        return _map_forward(x, weight, bias, H, W, eps, out_dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, weight, bias, H, W, eps, out_dtype = inputs
        y, mean, rstd = output
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mean, rstd)
        ctx.size = (H, W)
        ctx.save_for_backward(x, weight, mean, rstd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_mean, grad_rstd):
        wants = tuple(ctx.needs_input_grad[:3])
        if not any(wants) or grad_y is None:
            return (None,) * 7
        x, weight, mean, rstd = ctx.saved_tensors
        return _map_backward(grad_y, x, weight, mean, rstd, ctx.size[0], ctx.size[1], wants) + (None,) * 4


def layer_norm_to_map_composite(x, H, W, weight, bias, eps=1e-5, out_dtype=None):
    """What :func:`layer_norm_to_map` computes, by torch: the reference's ``norm_i(x_out)``, ``view``, ``permute`` and
    ``contiguous``."""
    y = F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    if out_dtype is not None:
        y = y.to(out_dtype)
    return y.view(-1, H, W, x.shape[-1]).permute(0, 3, 1, 2).contiguous()


def map_takes_kernels(x, weight, out_dtype):
    """Whether a call goes to the kernels: not while compiling, not on the CPU, not without elements, at most
    ``SWINENDS_MAX_CHANNELS`` channels and a dtype mix of include/swinends.h."""
    if torch.compiler.is_compiling() or not _on_gpu(x) or x.numel() == 0 or not 1 <= x.shape[-1] <= _swinends.MAX_CHANNELS:
        return False
    return map_supported(x.dtype, weight.dtype, x.dtype if out_dtype is None else out_dtype)


def layer_norm_to_map(x, H, W, weight, bias, eps=1e-5, out_dtype=None):
    """A stage's output norm as one HIP kernel pass (include/swinends.h): ``x [B, H * W, C]`` -> ``y [B, C, H, W]``, contiguous,
    ``y[b, :, h, w] = LayerNorm(x[b, h * W + w])`` -- bit for bit ``residual_layer_norm(x, None, weight, bias, eps)[1]``,
    permuted; ``C <= 3072``.  The normalised tokens never exist in token order: the transposition goes through LDS.

    dtypes: one of float32 / bfloat16 / float16 for all; a 16-bit ``out_dtype`` beside float32 ``x`` and parameters; float32
    parameters beside 16-bit tensors.  Differentiable in x, weight and bias (once); a gradient of ``y`` in another memory format
    (channels-last) is made dense on the host.  The composite route is :func:`patch_embed_norm`'s."""
    _require(x.dim() == 3 and x.shape[1] == H * W, "layer_norm_to_map: x must be [B, H * W, C], got %s for H, W = %d, %d" % (tuple(x.shape), H, W))
    C = x.shape[-1]
    _require(weight is not None and bias is not None and tuple(weight.shape) == (C,) and tuple(bias.shape) == (C,)
             and weight.dtype == bias.dtype, "layer_norm_to_map: weight and bias must be [%d] in one dtype" % C)
    if not map_takes_kernels(x, weight, out_dtype):
        return layer_norm_to_map_composite(x, H, W, weight, bias, eps, out_dtype)
    if _wants_grad(x, weight, bias):
        return LayerNormToMapFunction.apply(x, weight, bias, H, W, eps, out_dtype)[0]
    return _map_forward(x, weight, bias, H, W, eps, out_dtype, want_stats=False)[0]

"""The operator as ``torch.library`` custom ops (namespace ``devis_amd``), for ``torch.compile`` and ``torch.export``.

This module holds the op definitions, their fake implementations and the public wrappers.  Eager code never dispatches
through the ops (the deformable convolution, which has no other path, always does): the wrappers here call the autograd
Functions of :mod:`devis_amd.functions` and switch to the ops only while ``torch.compiler.is_compiling()`` (Dynamo tracing, or
export); the modules always call the four attention Functions, each of which picks the op or the host function once per
direction.  To the compiler each op is one opaque node whose implementation is that same host code -- the same checks, the same
kernels through the C ABI, the same numbers -- and whose fake implementation gives shapes and dtypes only.

An operator's autograd formula is written once, next to its host code in ``devis_amd/functions/<op>.py``: a
``setup_context(ctx, inputs, output)`` and a ``backward(run, ctx, *grads)`` whose ``run`` computes the gradients.  The eager
Function binds ``run`` to the host function; ``register_autograd`` here binds it to the backward op (``op_runner``: the
0-element tensors that stand for gradients not computed become None again).  Nothing in this module says what is saved or
where a gradient goes.  The ops:

=============================  ==========================================================================================
``ms_deform_attn_forward``     ``MSDeformAttnFunction`` forward (the im2col chunk loop), + the module's ``sum(H*W) == S``
``ms_deform_attn_backward``    ``MSDeformAttnFunction`` backward with every gradient -> (grad_value, grad_loc, grad_aw)
``temporal_forward/backward``  ``MSDeformAttnTemporalFunction``, likewise
``*_backward_grads``           the same two backwards with a ``grads`` mask (``_native.GRAD_VALUE`` / ``GRAD_SAMPLING``):
                               a group not asked for comes back as a tensor with 0 elements.  A formula names the full op
                               for ``GRAD_ALL`` and this one for a partial mask; both run the one host function, which
                               reaches the library through ``_native.backward_grads`` / ``temporal_backward_grads`` alone
``prep_forward/backward``      ``MSDeformPrepFunction`` (no temporal part: ``loc_t`` / ``aw_t`` come back with 0 slots)
``prep_fused_forward/backward``  ``MSDeformPrepFusedFunction``
``frame_table``                the temporal modules' frame table ``[T, W]`` int32 (cache and deferred range checks)
``deform_conv2d``              the mask head's modulated deformable convolution (:func:`deform_conv2d`, torchvision's
                               signature); ``deform_conv2d_backward`` computes the gradients its ``grads`` mask names
``deform_conv2d_pinned``       the same forward for a call that pins how its backward sums grad_input (the module's
                               ``reproducible_grad_input`` attribute): a constant of the graph, handed to the backward op
                               as a PIN_* bit of ``grads``
``attention_maps``             the mask head's attention maps (:func:`attention_maps`; include/attmap.h);
                               ``attention_maps_backward`` computes the gradients its ``grads`` mask names
``mask_head_stage``            one GroupNorm-ReLU-upsample-merge stage of the mask head (:func:`mask_head_stage`;
                               include/mhstage.h) -> (out in channels-last memory, mean, rstd);
                               ``mask_head_stage_backward`` computes the gradients its ``grads`` mask names
``mask_loss_terms``            the mask loss (:func:`mask_loss_terms`; include/maskloss.h) -> (focal [N], dice [N], the
                               [N, 3] sums the backward needs); ``mask_loss_terms_backward`` computes grad_src
``mask_soft_iou``              the clip-stitching cost (:func:`mask_soft_iou`; include/maskiou.h) -> (iou [Na, Nb], inter
                               [F, Na, Nb], sum_a [F, Na], sum_b [F, Nb]); an inference operator: no autograd formula
``binarize_masks``             the binarised full-resolution masks (:func:`binarize_masks`) -> bool [N, H, W]
``mask_run_lengths``           the COCO run lengths of those masks without the masks (:func:`mask_run_lengths`;
                               include/maskrle.h) -> int32 [N, 1 + max_runs]; an inference operator
``mask_binary_iou_terms``      the pixel counts of the binary clip-stitching cost (:func:`mask_binary_iou_terms`;
                               include/maskbiou.h) -> int32 (inter [Na, Nb, F], area_a [Na, F], area_b [Nb, F])
``mask_binary_iou``            the binary mask IoU matrix made of them (:func:`mask_binary_iou`) -> float64 [Na, Nb]; both
                               are inference operators
``match_cost``                 the Hungarian matchers' cost matrix (:func:`match_cost`; include/boxmatch.h) -> (cost
                               [L, R, T], status int32 [3]); no autograd formula
``box_loss_terms``             the box losses of matched pairs (:func:`box_loss_terms`) -> (l1 [N], giou [N]);
                               ``box_loss_terms_backward`` computes grad_src
``linear_assignment``          the assignment the matchers make of that cost (:func:`linear_assignment`; include/assign.h)
                               -> (rows int64 [L, n], cols int64 [L, n], status int32 [2]); no autograd formula
``label_loss_terms``           the criterion's label loss (:func:`label_loss_terms`; include/labelloss.h) -> (focal_sum [],
                               counts int32 [4], target_classes int32 [B, N]); ``label_loss_terms_backward`` computes
                               grad_logits
``sine_position_embedding``    the sine embedding of one padding mask (:func:`sine_position_embedding`; include/posembed.h)
                               -> pos [N, C, H, W]; no autograd formula
``encoder_position_embedding`` the encoder's positional input of all levels (:func:`encoder_position_embedding`) -> (pos
                               [N, S, C], mask_flatten bool [N, S], valid_ratios [N, L, 2]);
                               ``encoder_position_embedding_backward`` computes the gradients of the two embeddings
=============================  ==========================================================================================

Everything that reads the host or keeps Python state -- the ``spatial_shapes`` host hint, the frame-table cache, the
deferred verdicts of the temporal-offset range checks -- runs inside the implementations, at run time, never in a traced
graph.  The implementations look ``_native`` and ``ms_deform_attn_func._check_inputs`` up at call time.  The backward ops
carry no formula of their own: a second derivative raises, as ``once_differentiable`` does in eager.
Every op is tagged ``needs_fixed_stride_order``: Inductor hands over the strides eager would (e.g. the padded rows of
``value``) instead of contiguous copies.

When the package is imported a second time under another name (DeVIS's ``src.models.ops``), that copy registers its ops
under a namespace of its own (``devis_amd_src_models_ops``), bound to its own ``_native``.
"""
import functools
import re
from typing import List, Optional

import torch
from torch import Tensor

from . import _native
from .functions import assignment as _G
from .functions import attention_maps as _A
from .functions import box_matching as _X
from .functions import deform_conv as _D
from .functions import label_loss as _Y
from .functions import mask_binary_iou as _B
from .functions import mask_head_stage as _S
from .functions import mask_iou as _I
from .functions import mask_losses as _L
from .functions import mask_rle as _R
from .functions import ms_deform_attn_func as _F
from .functions import position_embedding as _P
from .functions._common import fill_slots, none_slots, op_runner


def _namespace():
    pkg = __name__.rsplit(".", 1)[0]
    base = "devis_amd" if pkg == "devis_amd" else "devis_amd_" + re.sub(r"\W", "_", pkg)
    ns, k = base, 1
    while hasattr(getattr(torch.ops, ns), "frame_table"):      # already taken (a re-import): the next free one
        ns, k = "%s_%d" % (base, k), k + 1
    return ns


NAMESPACE = _namespace()
_TAGS = (torch.Tag.needs_fixed_stride_order,)


def _op(name):
    return torch.library.custom_op("%s::%s" % (NAMESPACE, name), mutates_args=(), tags=_TAGS)


def _empty(like, shape, dtype=None):
    return torch.empty(shape, dtype=dtype or like.dtype, device=like.device)


# ---- MSDeformAttnFunction ------------------------------------------------------------------------------------------

@_op("ms_deform_attn_forward")
def ms_deform_attn_forward(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, sampling_loc: Tensor,
                           attn_weight: Tensor, im2col_step: int, padding_mask: Optional[Tensor] = None,
                           check_spatial_size: bool = False) -> Tensor:
    """``MSDeformAttnFunction.forward``.  ``check_spatial_size``: assert ``sum(H*W) == value.shape[1]`` as
    ``MSDeformAttn.forward`` does (ref ms_deform_attn.py:96), from the cached host copy of ``spatial_shapes``."""
    return _F._forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, padding_mask,
                       check_spatial_size)


@ms_deform_attn_forward.register_fake
def _(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, padding_mask=None,
      check_spatial_size=False):
    if padding_mask is not None:
        _F._require(padding_mask.dtype == torch.bool and padding_mask.numel() == value.shape[0] * value.shape[1],
                    "padding_mask must be a bool [N, S] tensor on value's device")
    _F._check_op_shapes(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    N, S, M, D = value.shape
    Lq = sampling_loc.shape[1]
    if N > 0 and Lq > 0:
        _F._im2col_step(N, im2col_step)
    return _empty(value, (N, Lq, M * D))


@_op("ms_deform_attn_backward")
def ms_deform_attn_backward(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, sampling_loc: Tensor,
                            attn_weight: Tensor, grad_output: Tensor, im2col_step: int,
                            padding_mask: Optional[Tensor] = None) -> tuple[Tensor, Tensor, Tensor]:
    """``MSDeformAttnFunction.backward``: (grad_value in value's dtype, grad_sampling_loc, grad_attn_weight)."""
    # (eager checks these once, in the forward; here the compiler chose what arrives)
    _F._check_inputs([("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                      ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)])
    return _F._backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step,
                        padding_mask)


@ms_deform_attn_backward.register_fake
def _(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step, padding_mask=None):
    return _empty(value, value.shape), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)


@_op("ms_deform_attn_backward_grads")
def ms_deform_attn_backward_grads(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, sampling_loc: Tensor,
                                  attn_weight: Tensor, grad_output: Tensor, im2col_step: int, grads: int,
                                  padding_mask: Optional[Tensor] = None) -> tuple[Tensor, Tensor, Tensor]:
    """``MSDeformAttnFunction.backward`` for the gradient groups in ``grads`` only; the others are 0-element tensors."""
    _F._check_inputs([("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                      ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)])
    out = _F._backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step,
                       padding_mask, grads)
    return fill_slots(out, _fake_backward_grads(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                                 grad_output, im2col_step, grads, padding_mask))


@ms_deform_attn_backward_grads.register_fake
def _fake_backward_grads(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step,
                         grads, padding_mask=None):
    _F._require(0 <= grads <= _native.GRAD_ALL, "grads must be a mask of GRAD_VALUE and GRAD_SAMPLING")
    v = grads & _native.GRAD_VALUE
    s = grads & _native.GRAD_SAMPLING
    return (_empty(value, value.shape if v else (0,)), _empty(sampling_loc, sampling_loc.shape if s else (0,)),
            _empty(attn_weight, attn_weight.shape if s else (0,)))


def run_ms_deform_attn_backward(value, shapes, lsi, loc, aw, grad_output, im2col_step, padding_mask, grads):
    """The two backward ops behind the signature of ``_F._backward``: what the formula runs in a compiled graph."""
    if grads == _native.GRAD_ALL:
        return ms_deform_attn_backward(value, shapes, lsi, loc, aw, grad_output, im2col_step, padding_mask)
    return none_slots(ms_deform_attn_backward_grads(value, shapes, lsi, loc, aw, grad_output, im2col_step, grads, padding_mask))


ms_deform_attn_forward.register_autograd(functools.partial(_F._backward_attn, run_ms_deform_attn_backward),
                                         setup_context=_F._setup_attn)


# ---- MSDeformAttnTemporalFunction ----------------------------------------------------------------------------------

@_op("temporal_forward")
def temporal_forward(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, frame_table: Tensor,
                     loc_curr: Tensor, aw_curr: Tensor, loc_temp: Tensor, aw_temp: Tensor, clips: int) -> Tensor:
    """``MSDeformAttnTemporalFunction.forward``: [clips*T, Lq, M*D]."""
    return _F._temporal_forward(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp,
                                aw_temp, clips)


@temporal_forward.register_fake
def _(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp, aw_temp, clips):
    _F._check_temporal_shapes(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp,
                              aw_temp, clips)
    G, S, M, D = value.shape
    return _empty(value, (G, loc_curr.shape[1], M * D))


@_op("temporal_backward")
def temporal_backward(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, frame_table: Tensor,
                      loc_curr: Tensor, aw_curr: Tensor, loc_temp: Tensor, aw_temp: Tensor, grad_output: Tensor,
                      clips: int) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """``MSDeformAttnTemporalFunction.backward``: (grad_value, grad_loc_curr, grad_aw_curr, grad_loc_temp, grad_aw_temp)."""
    _F._check_inputs([("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                      ("frame_table", frame_table), ("loc_curr", loc_curr), ("aw_curr", aw_curr), ("loc_temp", loc_temp),
                      ("aw_temp", aw_temp)])
    return _F._temporal_backward(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp,
                                 aw_temp, grad_output, clips)


@temporal_backward.register_fake
def _(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp, aw_temp, grad_output, clips):
    return (_empty(value, value.shape), torch.empty_like(loc_curr), torch.empty_like(aw_curr),
            torch.empty_like(loc_temp), torch.empty_like(aw_temp))


@_op("temporal_backward_grads")
def temporal_backward_grads(value: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, frame_table: Tensor,
                            loc_curr: Tensor, aw_curr: Tensor, loc_temp: Tensor, aw_temp: Tensor, grad_output: Tensor,
                            clips: int, grads: int) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """``MSDeformAttnTemporalFunction.backward`` for the gradient groups in ``grads`` only; the others are 0-element tensors."""
    _F._check_inputs([("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                      ("frame_table", frame_table), ("loc_curr", loc_curr), ("aw_curr", aw_curr), ("loc_temp", loc_temp),
                      ("aw_temp", aw_temp)])
    out = _F._temporal_backward(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp,
                                aw_temp, grad_output, clips, grads)
    return fill_slots(out, _fake_temporal_backward_grads(value, spatial_shapes, level_start_index, frame_table, loc_curr,
                                                          aw_curr, loc_temp, aw_temp, grad_output, clips, grads))


@temporal_backward_grads.register_fake
def _fake_temporal_backward_grads(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp,
                                  aw_temp, grad_output, clips, grads):
    _F._require(0 <= grads <= _native.GRAD_ALL, "grads must be a mask of GRAD_VALUE and GRAD_SAMPLING")
    v = grads & _native.GRAD_VALUE
    s = grads & _native.GRAD_SAMPLING
    return (_empty(value, value.shape if v else (0,)),) + tuple(_empty(t, t.shape if s else (0,))
                                                               for t in (loc_curr, aw_curr, loc_temp, aw_temp))


def run_temporal_backward(*args):
    """The two backward ops behind the signature of ``_F._temporal_backward`` (``grads`` last)."""
    if args[-1] == _native.GRAD_ALL:
        return temporal_backward(*args[:-1])
    return none_slots(temporal_backward_grads(*args))


temporal_forward.register_autograd(functools.partial(_F._backward_temporal, run_temporal_backward),
                                   setup_context=_F._setup_temporal)


# ---- MSDeformPrepFunction ------------------------------------------------------------------------------------------
# Outputs that do not exist without a temporal part (loc_t, aw_t and their gradients) are tensors with 0 slots here:
# a custom op returns tensors, not None.

def _prep_dims(off_c, off_t):
    R, M, L, Pc, _ = off_c.shape
    W = 0 if off_t is None else off_t.shape[2] // L
    Pt = 1 if off_t is None else off_t.shape[3]
    return R, M, L, W, Pc, Pt


@_op("prep_forward")
def prep_forward(off_c: Tensor, off_t: Optional[Tensor], logit_c: Tensor, logit_t: Optional[Tensor], ref_c: Tensor,
                 ref_t: Optional[Tensor], spatial_shapes: Tensor, loc32: bool = False
                 ) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``MSDeformPrepFunction.forward``: (loc_c, loc_t, aw_c, aw_t)."""
    (loc_c, loc_t, aw_c, aw_t), _ = _F._prep_forward(off_c, off_t, logit_c, logit_t, ref_c, ref_t, spatial_shapes, loc32)
    if loc_t is None:
        loc_t, aw_t = _fake_prep_forward(off_c, off_t, logit_c, logit_t, ref_c, ref_t, spatial_shapes, loc32)[1::2]
    return loc_c, loc_t, aw_c, aw_t


@prep_forward.register_fake
def _fake_prep_forward(off_c, off_t, logit_c, logit_t, ref_c, ref_t, spatial_shapes, loc32=False):
    R, M, L, W, Pc, Pt = _prep_dims(off_c, off_t)
    sdt = _F._sampling_dtype(off_c.dtype, loc32)
    _F._require(logit_c.dtype == off_c.dtype, "offsets / logits must share dtype and device")
    _F._require(tuple(ref_c.shape) == (R, L, ref_c.shape[-1]), "reference_points must be [rows, L, 2|4]")
    return (_empty(off_c, off_c.shape, sdt), _empty(off_c, (R, M, W * L, Pt, 2), sdt),
            _empty(off_c, (R, M, L, Pc), sdt), _empty(off_c, (R, M, W * L, Pt), sdt))


@_op("prep_backward")
def prep_backward(gloc_c: Optional[Tensor], gloc_t: Optional[Tensor], gaw_c: Optional[Tensor], gaw_t: Optional[Tensor],
                  aw_c: Tensor, aw_t: Optional[Tensor], off_c: Tensor, off_t: Optional[Tensor], ref_c: Tensor,
                  ref_t: Optional[Tensor], spatial_shapes: Tensor, loc32: bool = False, need_ref_c: bool = True,
                  need_ref_t: bool = True) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """``MSDeformPrepFunction.backward`` from the forward's INPUTS (``off_*``, ``ref_*`` as given) and ``aw_*`` outputs:
    (grad_off_c, grad_off_t, grad_logit_c, grad_logit_t, grad_ref_c, grad_ref_t); a reference-point gradient that is
    not asked for (``need_ref_*``) comes back with 0 elements."""
    args = (gloc_c, gloc_t, gaw_c, gaw_t, aw_c, aw_t, off_c, off_t, ref_c, ref_t, spatial_shapes, loc32, need_ref_c, need_ref_t)
    return fill_slots(_F._prep_backward(*args), _fake_prep_backward(*args))


@prep_backward.register_fake
def _fake_prep_backward(gloc_c, gloc_t, gaw_c, gaw_t, aw_c, aw_t, off_c, off_t, ref_c, ref_t, spatial_shapes,
                        loc32=False, need_ref_c=True, need_ref_t=True):
    R, M, L, W, Pc, Pt = _prep_dims(off_c, off_t)
    d = ref_c.shape[-1]
    return (_empty(off_c, off_c.shape), _empty(off_c, (R, M, W * L, Pt, 2)), _empty(off_c, (R, M, L * Pc)),
            _empty(off_c, (R, M, W * L * Pt)), _empty(ref_c, (R, L, d) if need_ref_c else (0,)),
            _empty(ref_c if ref_t is None else ref_t, (R, W * L, d) if (W and need_ref_t) else (0,)))


prep_forward.register_autograd(functools.partial(_F._backward_prep, prep_backward), setup_context=_F._setup_prep)


# ---- MSDeformPrepFusedFunction -------------------------------------------------------------------------------------

@_op("prep_fused_forward")
def prep_fused_forward(y: Tensor, ref_c: Tensor, ref_t: Optional[Tensor], spatial_shapes: Tensor, M: int, L: int, W: int,
                       Pc: int, Pt: int, loc32: bool = False) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``MSDeformPrepFusedFunction.forward``: (loc_c, loc_t, aw_c, aw_t)."""
    (loc_c, loc_t, aw_c, aw_t), _ = _F._prep_fused_forward(y, ref_c, ref_t, spatial_shapes, M, L, W, Pc, Pt, loc32)
    if not W:
        loc_t, aw_t = _fake_prep_fused_forward(y, ref_c, ref_t, spatial_shapes, M, L, W, Pc, Pt, loc32)[1::2]
    return loc_c, loc_t, aw_c, aw_t


@prep_fused_forward.register_fake
def _fake_prep_fused_forward(y, ref_c, ref_t, spatial_shapes, M, L, W, Pc, Pt, loc32=False):
    R = y.shape[0]
    cols = _F._prep_fused_cols(M, L, W, Pc, Pt)
    _F._require(y.dim() == 2 and y.shape[1] == cols[3][1], "y must be [rows, %d]" % cols[3][1])
    _F._require(tuple(ref_c.shape) == (R, L, ref_c.shape[-1]), "reference_points must be [rows, L, 2|4]")
    sdt = _F._sampling_dtype(y.dtype, loc32)
    return (_empty(y, (R, M, L, Pc, 2), sdt), _empty(y, (R, M, W * L, Pt, 2), sdt),
            _empty(y, (R, M, L, Pc), sdt), _empty(y, (R, M, W * L, Pt), sdt))


@_op("prep_fused_backward")
def prep_fused_backward(gloc_c: Optional[Tensor], gloc_t: Optional[Tensor], gaw_c: Optional[Tensor],
                        gaw_t: Optional[Tensor], aw_c: Tensor, aw_t: Optional[Tensor], y: Tensor, ref_c: Tensor,
                        ref_t: Optional[Tensor], spatial_shapes: Tensor, M: int, L: int, W: int, Pc: int, Pt: int,
                        loc32: bool = False, need_ref_c: bool = True, need_ref_t: bool = True
                        ) -> tuple[Tensor, Tensor, Tensor]:
    """``MSDeformPrepFusedFunction.backward`` from the forward's inputs and ``aw_*`` outputs: (grad_y, grad_ref_c,
    grad_ref_t); a reference-point gradient that is not asked for comes back with 0 elements."""
    args = (gloc_c, gloc_t, gaw_c, gaw_t, aw_c, aw_t, y, ref_c, ref_t, spatial_shapes, M, L, W, Pc, Pt, loc32, need_ref_c,
            need_ref_t)
    return fill_slots(_F._prep_fused_backward(*args), _fake_prep_fused_backward(*args))


@prep_fused_backward.register_fake
def _fake_prep_fused_backward(gloc_c, gloc_t, gaw_c, gaw_t, aw_c, aw_t, y, ref_c, ref_t, spatial_shapes, M, L, W, Pc, Pt,
                              loc32=False, need_ref_c=True, need_ref_t=True):
    R = y.shape[0]
    d = ref_c.shape[-1]
    return (_empty(y, (R, y.shape[1])), _empty(ref_c, (R, L, d) if need_ref_c else (0,)),
            _empty(ref_c if ref_t is None else ref_t, (R, W * L, d) if (W and need_ref_t) else (0,)))


prep_fused_forward.register_autograd(functools.partial(_F._backward_prep_fused, prep_fused_backward),
                                     setup_context=_F._setup_prep_fused)


# ---- frame table ---------------------------------------------------------------------------------------------------

@_op("frame_table")
def frame_table(offsets: List[Tensor], n_frames: int, device: torch.device) -> Tensor:
    """``TemporalMSDeformAttnBase._frame_table``: [T, W] int32 absolute frame ids on `device`.  Served from the frame-table
    cache and range-checked as in eager (IndexError; a pending verdict of an earlier device-side check is raised here)."""
    from .modules import ms_deform_attn as _mod
    # a copy: the compiled graph owns the op's output (Inductor may reuse its memory), the cache keeps its own
    return _mod._FRAME_TABLES.get(offsets, n_frames, torch.device(device)).clone()


@frame_table.register_fake
def _(offsets, n_frames, device):
    _F._require(len(offsets) > 0, "frame_table needs the temporal offsets of at least one frame")
    return torch.empty((n_frames, offsets[0].shape[0]), dtype=torch.int32, device=device)


# ---- modulated deformable convolution (include/mdcn.h) ---------------------------------------------------------------
# Unlike the attention operator this one has a single path: eager calls dispatch through the op too.

@_op("deform_conv2d")
def deform_conv2d_op(input: Tensor, offset: Tensor, weight: Tensor, bias: Optional[Tensor], stride: List[int],
                     padding: List[int], dilation: List[int], mask: Optional[Tensor]) -> Tensor:
    """``deform_conv2d`` with pairs for stride / padding / dilation: [N, Co, Ho, Wo]."""
    return _D._forward(input, offset, weight, bias, stride, padding, dilation, mask)


@deform_conv2d_op.register_fake
def _(input, offset, weight, bias, stride, padding, dilation, mask):
    Ho, Wo, _ = _D.check_shapes(input, offset, weight, bias, stride, padding, dilation, mask)
    return _empty(input, (input.shape[0], weight.shape[0], Ho, Wo))


@_op("deform_conv2d_backward")
def deform_conv2d_backward(grad_out: Tensor, input: Tensor, offset: Tensor, weight: Tensor, mask: Optional[Tensor],
                           stride: List[int], padding: List[int], dilation: List[int], grads: int
                           ) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(grad_input, grad_offset, grad_mask, grad_weight, grad_bias) for the gradients in ``grads`` (``NEED_*`` of
    devis_amd/functions/deform_conv.py); the others are 0-element tensors."""
    out = _D._backward(grad_out, input, offset, weight, mask, stride, padding, dilation, grads)
    return fill_slots(out, _fake_deform_conv2d_backward(grad_out, input, offset, weight, mask, stride, padding, dilation, grads))


@deform_conv2d_backward.register_fake
def _fake_deform_conv2d_backward(grad_out, input, offset, weight, mask, stride, padding, dilation, grads):
    _D._require(0 <= grads <= (_D.NEED_ALL | _D.PIN_BITS), "grads must be a mask of the NEED_* bits, with at most one PIN_* bit beside them")
    has = lambda bit, t: t is not None and bool(grads & bit)    # noqa: E731
    return (_empty(input, input.shape if has(_D.NEED_INPUT, input) else (0,)),
            _empty(offset, offset.shape if has(_D.NEED_OFFSET, offset) else (0,)),
            _empty(offset, mask.shape if has(_D.NEED_MASK, mask) else (0,)),
            _empty(weight, weight.shape if has(_D.NEED_WEIGHT, weight) else (0,)),
            _empty(weight, (weight.shape[0],) if grads & _D.NEED_BIAS else (0,)))


deform_conv2d_op.register_autograd(functools.partial(_D.backward, op_runner(deform_conv2d_backward)),
                                   setup_context=_D.setup_context)


# The process-wide switch of reproducible_grad_input is read inside the backward op, when it runs.  What ONE call pins has to
# be part of the graph instead (Python state around a call does not survive tracing): a forward op of its own carries it.
@_op("deform_conv2d_pinned")
def deform_conv2d_pinned_op(input: Tensor, offset: Tensor, weight: Tensor, bias: Optional[Tensor], stride: List[int],
                            padding: List[int], dilation: List[int], mask: Optional[Tensor],
                            reproducible_grad_input: bool) -> Tensor:
    """``deform_conv2d_op`` for a call whose backward sums grad_input in fixed point (True) or with float atomics (False)
    whatever the process-wide switch says.  The forward is the same."""
    return _D._forward(input, offset, weight, bias, stride, padding, dilation, mask)


@deform_conv2d_pinned_op.register_fake
def _(input, offset, weight, bias, stride, padding, dilation, mask, reproducible_grad_input):
    Ho, Wo, _ = _D.check_shapes(input, offset, weight, bias, stride, padding, dilation, mask)
    return _empty(input, (input.shape[0], weight.shape[0], Ho, Wo))


deform_conv2d_pinned_op.register_autograd(functools.partial(_D.backward, op_runner(deform_conv2d_backward)),
                                          setup_context=_D.setup_context)


def deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None, *,
                  reproducible_grad_input=None):
    """Modulated deformable convolution (DCNv2; DCNv1 with ``mask=None``) with the signature and semantics of
    ``torchvision.ops.deform_conv2d`` on the HIP kernels of include/mdcn.h: one weight group (anything else raises
    NotImplementedError), any number of offset groups, f32 / f64 / bf16 / f16 (``offset`` and ``mask`` may be float32 beside
    a 16-bit ``input``).  GPU tensors only.

    ``reproducible_grad_input`` (not torchvision's): None leaves the choice of grad_input's sum to
    :class:`devis_amd.reproducible_grad_input` when the backward runs; True / False pins this call to the order-independent
    fixed-point sum / to float atomics."""
    geometry = (list(_D._pair(stride, "stride")), list(_D._pair(padding, "padding")), list(_D._pair(dilation, "dilation")))
    if reproducible_grad_input is None:
        return deform_conv2d_op(input, offset, weight, bias, *geometry, mask)
    return deform_conv2d_pinned_op(input, offset, weight, bias, *geometry, mask, bool(reproducible_grad_input))


# ---- the mask head's attention maps (include/attmap.h) ---------------------------------------------------------------

@_op("attention_maps")
def attention_maps_op(q: Tensor, k: Tensor, mask: Optional[Tensor], num_heads: int, scale: float,
                      out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """``attention_maps`` with every argument given: [B, Q, n, H, W]."""
    return _A._forward(q, k, mask, num_heads, scale, out_dtype)


@attention_maps_op.register_fake
def _(q, k, mask, num_heads, scale, out_dtype=None):
    B, Q, n, c, H, W, odt = _A.check_shapes(q, k, mask, num_heads, out_dtype)
    return _empty(q, (B, Q, n, H, W), odt)


@_op("attention_maps_backward")
def attention_maps_backward(grad_out: Tensor, q: Tensor, k: Tensor, out: Tensor, num_heads: int, scale: float,
                            grads: int) -> tuple[Tensor, Tensor]:
    """(grad_q, grad_k) for the gradients in ``grads`` (``NEED_*`` of devis_amd/functions/attention_maps.py); the other
    is a 0-element tensor."""
    res = _A._backward(grad_out, q, k, out, num_heads, scale, grads)
    return fill_slots(res, _fake_attention_maps_backward(grad_out, q, k, out, num_heads, scale, grads))


@attention_maps_backward.register_fake
def _fake_attention_maps_backward(grad_out, q, k, out, num_heads, scale, grads):
    _A._require(0 <= grads <= _A.NEED_ALL, "grads must be a mask of NEED_Q and NEED_K")
    return (_empty(q, q.shape if grads & _A.NEED_Q else (0,)), _empty(k, k.shape if grads & _A.NEED_K else (0,)))


attention_maps_op.register_autograd(functools.partial(_A.backward, op_runner(attention_maps_backward)),
                                    setup_context=_A.setup_context)


def attention_maps(q, k, mask=None, *, num_heads, scale=None, out_dtype=None):
    """The attention maps of DeVIS's mask head (``MultiScaleMHAttentionMap``, one level) on the fused HIP kernels of
    include/attmap.h: ``softmax`` over all heads and pixels of ``scale * einsum("bqnc,bnchw->bqnhw", q, k)``, with the
    pixels where ``mask`` [B, H, W] is True at -inf.  ``q`` [B, Q, n*c], ``k`` [B, n*c, H, W] (f32 / f64 / bf16 / f16, the same
    for both) -> [B, Q, n, H, W] in ``out_dtype``: the inputs' dtype, or float32 beside 16-bit inputs.  ``scale`` defaults to
    ``c ** -0.5``.  A masked pixel is exactly 0; a row whose pixels are all masked is NaN.  GPU tensors only.  Every result is
    bitwise reproducible."""
    scale = _A.default_scale(q, num_heads) if scale is None else float(scale)
    if torch.compiler.is_compiling():
        return attention_maps_op(q, k, mask, num_heads, scale, out_dtype)
    return _A.AttentionMapsFunction.apply(q, k, mask, num_heads, scale, out_dtype)


# ---- one stage of the mask head's glue (include/mhstage.h) -------------------------------------------------------------

@_op("mask_head_stage")
def mask_head_stage_op(x: Tensor, num_groups: int, weight: Tensor, bias: Tensor, eps: float, skip: Optional[Tensor],
                       skip_index: Optional[Tensor], extra: Optional[Tensor],
                       out_dtype: Optional[torch.dtype] = None) -> tuple[Tensor, Tensor, Tensor]:
    """``mask_head_stage`` with every argument given: (out [N, C+E, H, W] in channels-last memory, mean, rstd [N, G])."""
    return _S._forward(x, num_groups, weight, bias, eps, skip, skip_index, extra, out_dtype)


@mask_head_stage_op.register_fake
def _(x, num_groups, weight, bias, eps, skip, skip_index, extra, out_dtype=None):
    N, F, C, G, E, h, w, H, W, odt = _S.check_shapes(x, num_groups, weight, bias, skip, skip_index, extra, out_dtype)
    acc = _native.acc_dtype(x.dtype)
    out = torch.empty((N, C + E, H, W), dtype=odt, device=x.device, memory_format=torch.channels_last)
    return out, _empty(x, (N, G), acc), _empty(x, (N, G), acc)


@_op("mask_head_stage_backward")
def mask_head_stage_backward(grad_out: Tensor, x: Tensor, weight: Tensor, bias: Tensor, mean: Tensor, rstd: Tensor,
                             skip_index: Optional[Tensor], num_groups: int, num_skip: int,
                             grads: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(grad_x, grad_weight, grad_bias, grad_skip) for the gradients in ``grads`` (``NEED_*`` of
    devis_amd/functions/mask_head_stage.py); the others are 0-element tensors.  ``num_skip`` is F."""
    res = _S._backward(grad_out, x, weight, bias, mean, rstd, skip_index, num_groups, num_skip, grads)
    return fill_slots(res, _fake_mask_head_stage_backward(grad_out, x, weight, bias, mean, rstd, skip_index, num_groups,
                                                           num_skip, grads))


@mask_head_stage_backward.register_fake
def _fake_mask_head_stage_backward(grad_out, x, weight, bias, mean, rstd, skip_index, num_groups, num_skip, grads):
    _S._require(0 <= grads <= _S.NEED_ALL, "grads must be a mask of the NEED_* bits")
    C, H, W = x.shape[1], grad_out.shape[2], grad_out.shape[3]
    return (_empty(x, x.shape if grads & _S.NEED_X else (0,)), _empty(weight, weight.shape if grads & _S.NEED_WEIGHT else (0,)),
            _empty(bias, bias.shape if grads & _S.NEED_BIAS else (0,)),
            _empty(x, (num_skip, C, H, W) if grads & _S.NEED_SKIP else (0,)))


mask_head_stage_op.register_autograd(functools.partial(_S.backward, op_runner(mask_head_stage_backward)),
                                     setup_context=_S.setup_context)


def mask_head_stage(x, num_groups, weight, bias, eps=1e-5, *, skip=None, skip_index=None, extra=None, out_dtype=None):
    """One stage of the glue of DeVIS's mask head (``MaskHeadConv``, between two of its convolutions) on the fused HIP
    kernels of include/mhstage.h::

        y   = relu(group_norm(x, num_groups, weight, bias, eps))                     x [N, C, h, w]
        y   = F.interpolate(y, size=(H, W), mode="nearest") + skip[skip_index]       skip [F, C, H, W], skip_index [N]
        out = cat([y, extra], 1)                                                     extra [N, E, H, W]

    ``skip``, ``skip_index`` (None: the identity, F == N) and ``extra`` are optional; (H, W) comes from ``skip``, else from
    ``extra``, else it is (h, w).  x and skip are f32 / f64 / bf16 / f16 alike; weight / bias, extra and ``out_dtype`` are
    that dtype, or float32 beside a 16-bit x.  ``out`` has the logical shape [N, C+E, H, W] in channels-last memory,
    always.  ``skip_index`` values outside [0, F) are the caller's contract (a device tensor is not read on the host).  GPU
    tensors only.  out and every gradient are bitwise reproducible."""
    if torch.compiler.is_compiling():
        return mask_head_stage_op(x, num_groups, weight, bias, float(eps), skip, skip_index, extra, out_dtype)[0]
    return _S.MaskHeadStageFunction.apply(x, num_groups, weight, bias, float(eps), skip, skip_index, extra, out_dtype)[0]


# ---- the mask loss (include/maskloss.h) --------------------------------------------------------------------------------

@_op("mask_loss_terms")
def mask_loss_terms_op(src: Tensor, target: Tensor, alpha: float, gamma: float) -> tuple[Tensor, Tensor, Tensor]:
    """``mask_loss_terms`` on [N, h, w] logits with every argument given: (focal [N], dice [N], sums [N, 3])."""
    return _L._forward(src, target, alpha, gamma)


@mask_loss_terms_op.register_fake
def _(src, target, alpha, gamma):
    N = _L.check_shapes(src, target)[0]
    _L.check_gamma(gamma)
    acc = _native.acc_dtype(src.dtype)
    return _empty(src, (N,), acc), _empty(src, (N,), acc), _empty(src, (N, 3), acc)


@_op("mask_loss_terms_backward")
def mask_loss_terms_backward(grad_focal: Tensor, grad_dice: Tensor, src: Tensor, target: Tensor, sums: Tensor,
                             alpha: float, gamma: float) -> Tensor:
    """grad_src [N, h, w] in src's dtype."""
    return _L._backward(grad_focal, grad_dice, src, target, sums, alpha, gamma)


@mask_loss_terms_backward.register_fake
def _(grad_focal, grad_dice, src, target, sums, alpha, gamma):
    return _empty(src, src.shape)


mask_loss_terms_op.register_autograd(functools.partial(_L.backward, mask_loss_terms_backward), setup_context=_L.setup_context)


def mask_loss_terms(src_masks, target_masks, alpha=0.25, gamma=2.0):
    """The per-instance terms of DeVIS's mask loss (``SetCriterion.loss_masks``) on the fused HIP kernels of
    include/maskloss.h::

        x     = F.interpolate(src_masks[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0].flatten(1)
        t     = target_masks.flatten(1).to(x)
        focal = sigmoid_focal_loss(x, t, alpha, gamma) without its reduction over instances: the mean over pixels, [N]
        dice  = 1 - (2 * (x.sigmoid() * t).sum(1) + 1) / (x.sigmoid().sum(1) + t.sum(1) + 1)                     [N]

    ``src_masks`` [N, h, w] or [N, 1, h, w] logits (f32 / f64 / bf16 / f16), ``target_masks`` [N, H, W]: bool or uint8
    (nonzero is 1; one byte per pixel is all the operator reads), or floating -- float32 or the logits' dtype -- taken as it
    is.  The results are float32 (float64 for float64 logits), also under autocast, which leaves the logits as they are.
    ``alpha < 0`` switches the class weighting off; ``gamma`` is 0, 1 or larger than 1 (ValueError otherwise).  Only
    ``src_masks`` has a gradient; a floating target that requires one raises.  Nothing of the target's resolution is
    allocated, forward or backward.  GPU tensors only.  Every result is bitwise reproducible."""
    gamma = _L.check_gamma(gamma)
    if src_masks.dim() == 4:
        _L._require(src_masks.shape[1] == 1, "mask_loss_terms: src_masks must be [N, h, w] or [N, 1, h, w], got %s"
                    % (tuple(src_masks.shape),))
        src_masks = src_masks[:, 0]
    _L._require(not (target_masks.is_floating_point() and target_masks.requires_grad),
                "mask_loss_terms: target_masks has no gradient (detach it)")
    if torch.compiler.is_compiling():
        return mask_loss_terms_op(src_masks, target_masks, float(alpha), gamma)[:2]
    return _L.MaskLossTermsFunction.apply(src_masks, target_masks, float(alpha), gamma)[:2]


def mask_losses(src_masks, target_masks, num_boxes, alpha=0.25, gamma=2.0):
    """DeVIS's pair of mask losses from the matched logit maps and their targets: ``{"loss_mask": sum of the focal terms /
    num_boxes, "loss_dice": sum of the dice terms / num_boxes}`` of :func:`mask_loss_terms`.  ``num_boxes`` is a number or a
    tensor, as in the reference; the two tiny reductions stay in torch."""
    focal, dice = mask_loss_terms(src_masks, target_masks, alpha, gamma)
    return {"loss_mask": focal.sum() / num_boxes, "loss_dice": dice.sum() / num_boxes}


# ---- clip stitching (include/maskiou.h) --------------------------------------------------------------------------------

@_op("mask_soft_iou")
def mask_soft_iou_op(a: Tensor, b: Tensor, size: List[int], reduce: str, eps: float) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``mask_soft_iou`` on [N, F, h, w] logits with every argument given: (iou, inter, sum_a, sum_b)."""
    return _I._pairwise(a, b, size, reduce, eps)


@mask_soft_iou_op.register_fake
def _(a, b, size, reduce, eps):
    Na, Nb, F = _I.check_pair(a, b, size)[:3]
    _I.check_reduce(reduce)
    _I.check_eps(eps)
    acc = _native.acc_dtype(a.dtype)
    return _empty(a, (Na, Nb), acc), _empty(a, (F, Na, Nb), acc), _empty(a, (F, Na), acc), _empty(a, (F, Nb), acc)


@_op("binarize_masks")
def binarize_masks_op(src: Tensor, size: List[int], order: str) -> Tensor:
    """``binarize_masks`` with every argument given: bool [N, H, W] (for "F" the transposed view of a dense [N, W, H])."""
    return _I._binarize(src, size, order)


@binarize_masks_op.register_fake
def _(src, size, order):
    N, _h, _w, H, W = _I.check_src(src, size)
    _I.check_order(order)
    if order == "F":
        return _empty(src, (N, W, H), torch.bool).transpose(1, 2)
    return _empty(src, (N, H, W), torch.bool)


def _stitch_args(a, b):
    _I._require(a.dim() == b.dim() and a.dim() in (3, 4), "mask_soft_iou: a and b must be [N, F, h, w] (or [N, h, w])")
    _I.check_no_grad("mask_soft_iou", [("a", a), ("b", b)])
    return (a[:, None], b[:, None]) if a.dim() == 3 else (a, b)


def _soft_iou(a, b, size, reduce, eps):
    a, b = _stitch_args(a, b)
    size = [size[0], size[1]] if len(size) == 2 else list(size)
    if torch.compiler.is_compiling():
        return mask_soft_iou_op(a, b, size, reduce, eps)
    with torch.no_grad():
        return _I._pairwise(a, b, size, reduce, eps)


def mask_soft_iou(a, b, size, *, reduce="volume", eps=1e-6):
    """The soft mask IoU between every map of ``a`` and every map of ``b`` -- DeVIS's clip-stitching cost
    (``HungarianInferenceMatcher.soft_iou`` over all pairs) -- on the fused HIP kernels of include/maskiou.h::

        pa = F.interpolate(a, size=size, mode="bilinear", align_corners=False).sigmoid().flatten(2)      # [Na, F, H*W]
        pb = likewise                                                                                     # [Nb, F, H*W]
        inter = einsum("ifk,jfk->fij", pa, pb);  sa = pa.sum(2).T;  sb = pb.sum(2).T
        "volume":  I, Sa, Sb = the sums over f;  I / (Sa[:, None] + Sb[None] - I).clamp(min=eps)
        "frame":   (inter / (sa[:, :, None] + sb[:, None] - inter).clamp(min=eps)).mean(0)

    ``a`` [Na, F, h, w] and ``b`` [Nb, F, h, w] logits (or [N, h, w]: one frame) of one dtype (f32 / f64 / bf16 / f16);
    ``size`` the (H, W) both are resampled to.  Returns [Na, Nb] in float32 (float64 for float64 logits).  The probability
    maps never exist in memory.  An inference operator: no gradient, and an input that requires one while gradients are
    recorded raises.  GPU tensors only.  Bitwise reproducible; an entry has the same bits alone and in any larger call."""
    return _soft_iou(a, b, size, _I.check_reduce(reduce), _I.check_eps(eps))[0]


def mask_soft_iou_terms(a, b, size):
    """``(inter [F, Na, Nb], sum_a [F, Na], sum_b [F, Nb])`` of :func:`mask_soft_iou`: per frame the sum over the pixels of
    the product of the two probability maps, and of each map's probabilities."""
    return tuple(_soft_iou(a, b, size, "volume", 1e-6)[1:])


def binarize_masks(src, size, *, order="C"):
    """``F.interpolate(src[:, None], size=size, mode="bilinear", align_corners=False)[:, 0] > 0`` as bool [N, H, W] on the
    HIP kernel of include/maskiou.h: the reference's ``sigmoid() > 0.5`` without the float map (the two differ only for
    logits between 0 and about 6e-8).  ``src`` [N, h, w] logits (f32 / f64 / bf16 / f16).  ``order="F"`` returns the
    transposed view of a dense [N, W, H] buffer: every mask in Fortran order, as a run-length encoder reads it.  NaN gives
    False.  An inference operator: no gradient.  GPU tensors only."""
    order = _I.check_order(order)
    _I.check_no_grad("binarize_masks", [("src", src)])
    size = [size[0], size[1]] if len(size) == 2 else list(size)
    if torch.compiler.is_compiling():
        return binarize_masks_op(src, size, order)
    with torch.no_grad():
        return _I._binarize(src, size, order)


# ---- the run-length encoder (include/maskrle.h) --------------------------------------------------------------------------

@_op("mask_run_lengths")
def mask_run_lengths_op(src: Tensor, size: List[int], max_runs: int) -> Tensor:
    """``mask_run_lengths`` with every argument given: int32 [N, 1 + max_runs]."""
    return _R._run_lengths(src, size, max_runs)


@mask_run_lengths_op.register_fake
def _(src, size, max_runs):
    N = _R.check_src(src, size, max_runs)[0]
    return _empty(src, (N, 1 + max_runs), torch.int32)


def mask_run_lengths(src, size, *, max_runs=None):
    """The COCO run lengths of ``binarize_masks(src, size)`` on the HIP kernels of include/maskrle.h, without the byte map:
    int32 ``runs`` [N, 1 + max_runs] from ``src`` [N, h, w] logits (f32 / f64 / bf16 / f16).  Every mask is walked in
    column-major order; its counts are the lengths of the alternating runs of equal bits, the first a run of zeros (0 when
    pixel (0, 0) is set): what ``{"size": [H, W], "counts": [...]}`` holds in an uncompressed COCO encoding.
    ``runs[n, 0]`` is the mask's number of runs R_n -- the true one, also when it exceeds ``max_runs`` --
    ``runs[n, 1:1 + min(R_n, max_runs)]`` the counts or their prefix, and the rest of the row 0.  A row with
    ``R_n > max_runs`` is truncated and must not be decoded.  ``max_runs`` defaults to ``min(H*W + 1, 8*W + 1)``; a compact
    region has at most ``2*W + 1`` runs.  The bits are those of :func:`binarize_masks` at every pixel (NaN gives 0).  An
    inference operator: no gradient.  GPU tensors only.  A mask has the same row alone and in any batch."""
    size = [size[0], size[1]] if len(size) == 2 else list(size)
    if max_runs is None:            # (the other checks of size are the operator's: nothing here formats a symbolic size)
        _R._require(len(size) == 2, "mask_run_lengths: size must be (H, W)")
        max_runs = _R.default_max_runs(size[0], size[1])
    else:
        _R.check_max_runs(max_runs)
    _I.check_no_grad("mask_run_lengths", [("src", src)])
    if torch.compiler.is_compiling():
        return mask_run_lengths_op(src, size, max_runs)
    with torch.no_grad():
        return _R._run_lengths(src, size, max_runs)


# ---- the binary mask IoU (include/maskbiou.h) ----------------------------------------------------------------------------

@_op("mask_binary_iou_terms")
def mask_binary_iou_terms_op(a: Tensor, b: Tensor, size: List[int]) -> tuple[Tensor, Tensor, Tensor]:
    """``mask_binary_iou_terms`` on [N, F, h, w] logits: int32 (inter [Na, Nb, F], area_a [Na, F], area_b [Nb, F])."""
    return _B._terms(a, b, size)


@mask_binary_iou_terms_op.register_fake
def _(a, b, size):
    Na, Nb, F = _B.check_pair(a, b, size)[:3]
    return _empty(a, (Na, Nb, F), torch.int32), _empty(a, (Na, F), torch.int32), _empty(a, (Nb, F), torch.int32)


@_op("mask_binary_iou")
def mask_binary_iou_op(a: Tensor, b: Tensor, size: List[int], reduce: str) -> Tensor:
    """``mask_binary_iou`` with every argument given: float64 [Na, Nb]."""
    return _B._binary_iou(a, b, size, reduce)


@mask_binary_iou_op.register_fake
def _(a, b, size, reduce):
    Na, Nb = _B.check_pair(a, b, size)[:2]
    _B.check_reduce(reduce)
    return _empty(a, (Na, Nb), torch.float64)


def mask_binary_iou_terms(a, b, size):
    """The pixel counts a binary mask IoU is made of, between every map of ``a`` and every map of ``b``, on the HIP kernels of
    include/maskbiou.h: int32 ``(inter [Na, Nb, F], area_a [Na, F], area_b [Nb, F])`` from ``a`` [Na, F, h, w] and ``b``
    [Nb, F, h, w] logits of one dtype (f32 / f64 / bf16 / f16)::

        A = binarize_masks(a.flatten(0, 1), size).view(Na, F, H*W);  B likewise
        inter[i, j, f] = (A[i, f] & B[j, f]).sum();  area_a[i, f] = A[i, f].sum();  area_b[j, f] = B[j, f].sum()

    The bits are those of :func:`binarize_masks` at every pixel (NaN gives 0); the byte maps never exist in memory -- a mask
    is one bit per pixel in the workspace, and an intersection a population count.  The counts are exact integers.  An
    inference operator: no gradient.  GPU tensors only.  A pair has the same counts alone and in any larger call."""
    _I.check_no_grad("mask_binary_iou", [("a", a), ("b", b)])
    size = [size[0], size[1]] if len(size) == 2 else list(size)
    if torch.compiler.is_compiling():
        return mask_binary_iou_terms_op(a, b, size)
    with torch.no_grad():
        return _B._terms(a, b, size)


def mask_binary_iou(a, b, size, *, reduce="volume"):
    """The IoU of the binarised full-resolution masks between every map of ``a`` and every map of ``b`` -- DeVIS's
    clip-stitching cost with ``use_binary_mask_iou`` (``HungarianInferenceMatcher.iou`` over all pairs) -- as float64
    [Na, Nb], formed on the device in int64 from :func:`mask_binary_iou_terms`::

        "volume":  I = inter.sum(2);  U = area_a.sum(1)[:, None] + area_b.sum(1)[None] - I;  I / U, 0.0 where U == 0
        "frame":   the mean over f of inter / (area_a[:, None] + area_b[None] - inter), each 0.0 where its union is 0

    ``"frame"`` is ``compute_frame_average_iou_cost`` with ``compute_iou_matrix``.  The counts are exact, so a ratio is the
    correctly rounded quotient of two integers.  An inference operator: no gradient.  GPU tensors only."""
    reduce = _B.check_reduce(reduce)
    _I.check_no_grad("mask_binary_iou", [("a", a), ("b", b)])
    size = [size[0], size[1]] if len(size) == 2 else list(size)
    if torch.compiler.is_compiling():
        return mask_binary_iou_op(a, b, size, reduce)
    with torch.no_grad():
        return _B._binary_iou(a, b, size, reduce)


# ---- the criterion's matching cost and box losses (include/boxmatch.h) ----------------------------------------------------

@_op("match_cost")
def match_cost_op(logits: Tensor, boxes: Tensor, tgt_labels: Tensor, tgt_boxes: Tensor, cost_class: float, cost_bbox: float,
                  cost_giou: float, l1: str, alpha: float) -> tuple[Tensor, Tensor]:
    """``match_cost`` with every argument given: (cost [L, R, T], status int32 [3])."""
    return _X._match_cost(logits, boxes, tgt_labels, tgt_boxes, cost_class, cost_bbox, cost_giou, l1, alpha)


@match_cost_op.register_fake
def _(logits, boxes, tgt_labels, tgt_boxes, cost_class, cost_bbox, cost_giou, l1, alpha):
    L, _F_, R, T = _X.check_match(logits, boxes, tgt_labels, tgt_boxes)[:4]
    _X.check_l1(l1)
    return _empty(logits, (L, R, T), _native.acc_dtype(logits.dtype)), _empty(logits, (3,), torch.int32)


def match_cost(logits, boxes, tgt_labels, tgt_boxes, *, cost_class=1.0, cost_bbox=1.0, cost_giou=1.0, l1="mean", alpha=0.25):
    """The cost matrix DeVIS's Hungarian matchers hand to the assignment solver (``DeVISHungarianMatcher.forward``,
    ``HungarianMatcher.forward`` with ``focal_loss``) on the HIP kernel of include/boxmatch.h, for ``L`` independent problems
    of ``R`` rows and ``T`` targets over ``F`` frames::

        cost[l, r, t] = cost_class * mean_f cls(logits[l, f, r, tgt_labels[t, f]])
                      + cost_bbox  * L1(boxes[l, :, r], tgt_boxes[t])
                      + cost_giou  * (-mean_f GIoU(boxes[l, f, r], tgt_boxes[t, f]))
        cls(x) = alpha * (1-p)^2 * (-log(p + 1e-8)) - (1-alpha) * p^2 * (-log(1 - p + 1e-8)),  p = sigmoid(x)

    ``logits`` [L, F, R, C] and ``boxes`` [L, F, R, 4] (cxcywh) of one dtype (f32 / f64 / bf16 / f16), ``tgt_labels`` int64
    [T, F], ``tgt_boxes`` [T, F, 4] in that dtype or float32 beside a 16-bit one.  ``l1`` is ``"mean"`` (the mean over frames
    and coordinates of ``|box - tgt|``) or ``"sum"`` (the mean over frames of the sum over coordinates: ``cdist(p=1)``,
    DeVIS's ``USE_SUM_L1_DISTANCE``).  GIoU is the reference's ``generalized_box_iou`` with its ``1e-6`` terms.

    Returns ``(cost [L, R, T], status int32 [3])``, ``cost`` in float32 (float64 for float64 inputs).  ``status`` counts,
    without a synchronisation, what the reference asserts on: [0] prediction boxes and [1] target boxes with ``x1 < x0`` or
    ``y1 < y0``, [2] labels outside ``[0, C)`` -- such a label is never used as an index, and its entries are NaN.  A NaN
    input gives NaN in the entries that read it and nowhere else.  No gradient: an input that requires one while gradients
    are recorded raises.  GPU tensors only.  One launch, no workspace; an entry has the same bits alone and in any larger
    call."""
    l1 = _X.check_l1(l1)
    _I.check_no_grad("match_cost", [("logits", logits), ("boxes", boxes), ("tgt_boxes", tgt_boxes)])
    args = (float(cost_class), float(cost_bbox), float(cost_giou), l1, float(alpha))
    if torch.compiler.is_compiling():
        return match_cost_op(logits, boxes, tgt_labels, tgt_boxes, *args)
    with torch.no_grad():
        return _X._match_cost(logits, boxes, tgt_labels, tgt_boxes, *args)


@_op("box_loss_terms")
def box_loss_terms_op(src: Tensor, target: Tensor) -> tuple[Tensor, Tensor]:
    """``box_loss_terms`` as an op: (l1 [N], giou [N])."""
    return _X._forward(src, target)


@box_loss_terms_op.register_fake
def _(src, target):
    N = _X.check_pairs(src, target)[0]
    acc = _native.acc_dtype(src.dtype)
    return _empty(src, (N,), acc), _empty(src, (N,), acc)


@_op("box_loss_terms_backward")
def box_loss_terms_backward(grad_l1: Tensor, grad_giou: Tensor, src: Tensor, target: Tensor) -> Tensor:
    """grad_src [N, 4] in src's dtype."""
    return _X._backward(grad_l1, grad_giou, src, target)


@box_loss_terms_backward.register_fake
def _(grad_l1, grad_giou, src, target):
    return _empty(src, src.shape)


box_loss_terms_op.register_autograd(functools.partial(_X.backward, box_loss_terms_backward), setup_context=_X.setup_context)


def box_loss_terms(src_boxes, target_boxes):
    """The per-pair terms of DeVIS's box losses (``SetCriterion.loss_boxes``) on the HIP kernels of include/boxmatch.h::

        l1   = F.l1_loss(src_boxes, target_boxes, reduction="none").sum(1)                                        [N]
        giou = 1 - diag(generalized_box_iou(box_cxcywh_to_xyxy(src_boxes), box_cxcywh_to_xyxy(target_boxes)))     [N]

    without the N x N matrix.  ``src_boxes`` [N, 4] cxcywh (f32 / f64 / bf16 / f16), ``target_boxes`` [N, 4] in that dtype or
    float32 beside a 16-bit one.  The results are float32 (float64 for float64 boxes).  Only ``src_boxes`` has a gradient --
    torch autograd's, also at the ties of ``max`` / ``min`` (halves), at ``clamp(min=0)`` (passes at 0) and at ``|0|`` (0);
    a target that requires one raises; there is no double backward.  Forward and backward are one launch each.  The
    reference's two degenerate-box asserts are not reproduced.  GPU tensors only.  Every result is bitwise reproducible."""
    _X._require(not target_boxes.requires_grad, "box_loss_terms: target_boxes has no gradient (detach it)")
    if torch.compiler.is_compiling():
        return box_loss_terms_op(src_boxes, target_boxes)
    return _X.BoxLossTermsFunction.apply(src_boxes, target_boxes)


def box_losses(src_boxes, target_boxes, num_boxes):
    """DeVIS's pair of box losses from the matched boxes: ``{"loss_bbox": sum of the L1 terms / num_boxes, "loss_giou": sum of
    the GIoU terms / num_boxes}`` of :func:`box_loss_terms`.  ``num_boxes`` is a number or a tensor, as in the reference; the
    two tiny reductions stay in torch."""
    l1, giou = box_loss_terms(src_boxes, target_boxes)
    return {"loss_bbox": l1.sum() / num_boxes, "loss_giou": giou.sum() / num_boxes}


# ---- the matchers' assignment (include/assign.h) ---------------------------------------------------------------------------

@_op("linear_assignment")
def linear_assignment_op(cost: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """``linear_assignment`` as an op: (rows int64 [L, n], cols int64 [L, n], status int32 [2])."""
    return _G._solve(cost)


@linear_assignment_op.register_fake
def _(cost):
    L, R, T = _G.check_cost(cost)
    n = torch.sym_min(R, T)
    return _empty(cost, (L, n), torch.int64), _empty(cost, (L, n), torch.int64), _empty(cost, (2,), torch.int32)


def linear_assignment(cost):
    """``scipy.optimize.linear_sum_assignment`` of ``L`` independent problems on the HIP kernel of include/assign.h, without a
    transfer: ``cost`` [L, R, T] in float32 or float64 -- :func:`match_cost`'s output as it lies -- gives
    ``(rows [L, n], cols [L, n], status int32 [2])`` with ``n = min(R, T)``, int64 indices on ``cost``'s device, the pairs of a
    problem ordered by ascending row as scipy orders them.  The method is scipy's (the shortest augmenting paths of Crouse
    2016) in double; among columns of equal shortest-path value one without a row is taken first, then the lowest index, so a
    unique optimum gives scipy's indices and a tied one gives an assignment of scipy's total.

    ``status`` counts, without a synchronisation, the problems scipy raises on: [0] those with a NaN or ``-inf`` entry
    ("matrix contains invalid numeric entries"), [1] those ``+inf`` entries make infeasible ("cost matrix is infeasible").
    Such a problem gets the pairs ``(k, k)``; the others are unaffected.  :func:`devis_amd.raise_on_match_status` reads the
    counts and raises.  Sides up to 1024.  No gradient: an input that requires one while gradients are recorded raises.
    GPU tensors only.  One launch of one wave per problem; the result is bitwise reproducible, and a problem has the same one
    alone and in any larger call."""
    _I.check_no_grad("linear_assignment", [("cost", cost)])
    if torch.compiler.is_compiling():
        return linear_assignment_op(cost)
    with torch.no_grad():
        return _G._solve(cost)


# ---- the criterion's label loss (include/labelloss.h) ----------------------------------------------------------------------

@_op("label_loss_terms")
def label_loss_terms_op(logits: Tensor, rows: Tensor, labels: Tensor, valid: Optional[Tensor],
                        alpha: float) -> tuple[Tensor, Tensor, Tensor]:
    """``label_loss_terms`` with every argument given: (focal_sum [], counts int32 [4], target_classes int32 [B, N])."""
    return _Y._forward(logits, rows, labels, valid, alpha)


@label_loss_terms_op.register_fake
def _(logits, rows, labels, valid, alpha):
    B, N = _Y.check_labels(logits, rows, labels, valid)[:2]
    return (_empty(logits, (), _native.acc_dtype(logits.dtype)), _empty(logits, (4,), torch.int32),
            _empty(logits, (B, N), torch.int32))


@_op("label_loss_terms_backward")
def label_loss_terms_backward(grad_sum: Tensor, logits: Tensor, target_classes: Tensor, alpha: float) -> Tensor:
    """grad_logits [B, N, C] in logits' dtype."""
    return _Y._backward(grad_sum, logits, target_classes, alpha)


@label_loss_terms_backward.register_fake
def _(grad_sum, logits, target_classes, alpha):
    return _empty(logits, logits.shape)


label_loss_terms_op.register_autograd(functools.partial(_Y.backward, label_loss_terms_backward), setup_context=_Y.setup_context)


def label_loss_terms(logits, rows, labels, valid=None, *, alpha=0.25):
    """The terms of DeVIS's label loss (``SetCriterion.loss_labels_focal``) on the fused HIP kernels of
    include/labelloss.h, from the matcher's index tensors as they lie::

        target_classes = full([B, N], C);  target_classes.view(-1)[rows[valid]] = labels[valid]
        focal_sum = sigmoid_focal_loss(logits, one_hot(target_classes, C + 1)[..., :C], alpha, gamma=2) summed over all elements
        counts    = [matches, matches whose query's argmax is their label, bad rows, bad labels]

    ``logits`` [B, N, C] (f32 / f64 / bf16 / f16), ``rows`` int64 [M] -- the flattened query ``b * N + src`` of each match --,
    ``labels`` int64 [M], ``valid`` bool or uint8 [M] or None for all valid: a tensor operand, not a boolean index.  A match
    counts when it is valid, ``0 <= row < B * N`` and ``0 <= label <= C`` (``C`` is "no object": counted, no positive); the
    others are ignored.  Of several matches of one query the one with the highest position wins (``index_put_``'s order on
    the CPU).  ``alpha < 0`` switches the class weighting off.

    Returns ``(focal_sum [], counts int32 [4], target_classes int32 [B, N])``, ``focal_sum`` in float32 (float64 for float64
    logits).  ``counts[1]`` takes the lowest class index on a tie, and a query with a NaN logit is never correct;
    ``counts[2]`` / ``counts[3]`` are the valid matches with a row outside ``[0, B * N)`` / a label outside ``[0, C]``.  Only
    ``focal_sum`` is differentiable, and only with respect to ``logits``; there is no double backward.  The forward is one
    launch (two beyond ``labelloss_tile`` logits), the backward one; no one-hot tensor is allocated and no call synchronises.
    GPU tensors only.  Every result is bitwise reproducible and does not depend on the order of the matches."""
    if logits.requires_grad:
        _native.dtype_code(logits.dtype)       # (raises on a dtype the unit lacks)
    if torch.compiler.is_compiling():
        return label_loss_terms_op(logits, rows, labels, valid, float(alpha))
    return _Y.LabelLossTermsFunction.apply(logits, rows, labels, valid, float(alpha))


def label_losses(logits, rows, labels, valid, num_boxes, *, alpha=0.25, log=True):
    """DeVIS's label loss from the logits and the matcher's indices: ``{"loss_ce": focal_sum / num_boxes}`` of
    :func:`label_loss_terms` and, with ``log``, ``"class_error"``: 100 minus the matched queries' top-1 accuracy in percent
    -- the reference's ``accuracy``, 0 for no matches included -- as a device scalar, without a synchronisation.
    ``num_boxes`` is a number or a tensor, as in the reference; the division stays in torch."""
    focal_sum, counts, _ = label_loss_terms(logits, rows, labels, valid, alpha=alpha)
    losses = {"loss_ce": focal_sum / num_boxes}
    if log:
        matched, correct = counts[0], counts[1]
        losses["class_error"] = 100 - torch.where(matched > 0, 100 * correct / matched, torch.zeros_like(focal_sum))
    return losses


# ---- the encoder's positional input (include/posembed.h) -------------------------------------------------------------------

@_op("sine_position_embedding")
def sine_position_embedding_op(mask: Tensor, num_pos_feats: int, temperature: float, normalize: bool, scale: Optional[float],
                               out_dtype: Optional[torch.dtype]) -> Tensor:
    """``sine_position_embedding`` with every argument given: pos [N, 2 * num_pos_feats, H, W]."""
    return _P._sine(mask, num_pos_feats, temperature, normalize, scale, out_dtype)


@sine_position_embedding_op.register_fake
def _(mask, num_pos_feats, temperature, normalize, scale, out_dtype):
    N, (H, W), _, out_dtype = _P.check_sine(mask, num_pos_feats, normalize, scale, out_dtype)
    return _empty(mask, (N, 2 * num_pos_feats, H, W), out_dtype)


def sine_position_embedding(mask, *, num_pos_feats, temperature=10000, normalize=False, scale=None, out_dtype=None):
    """DeVIS's ``PositionEmbeddingSine.forward`` of a padding mask on the HIP kernels of include/posembed.h::

        y_embed, x_embed = (~mask).cumsum(1), (~mask).cumsum(2)          # then, with normalize, / (last + 1e-6) * scale
        pos = cat(sin | cos of y_embed / dim_t, sin | cos of x_embed / dim_t).permute(0, 3, 1, 2)

    ``mask`` bool [N, H, W] with any strides (True is padding); ``num_pos_feats`` even; ``scale`` (default ``2 * pi``) needs
    ``normalize``; ``out_dtype`` float32 (the default), bfloat16 or float16: float32 arithmetic with the reference's
    operations in the reference's order, rounded once at the store.  Returns ``[N, 2 * num_pos_feats, H, W]``, without a
    gradient (a mask has none).  Two launches: the counts -- integer prefix sums by wave ballots -- and the write pass.  GPU
    tensors only."""
    if torch.compiler.is_compiling():
        return sine_position_embedding_op(mask, num_pos_feats, float(temperature), bool(normalize), scale, out_dtype)
    with torch.no_grad():
        return _P._sine(mask, num_pos_feats, float(temperature), bool(normalize), scale, out_dtype)


@_op("encoder_position_embedding")
def encoder_position_embedding_op(masks: List[Tensor], level_embed: Tensor, temporal_embed: Optional[Tensor],
                                  num_pos_feats: Optional[int], temperature: float, normalize: bool, scale: Optional[float],
                                  round_dtype: Optional[torch.dtype],
                                  out_dtype: Optional[torch.dtype]) -> tuple[Tensor, Tensor, Tensor]:
    """``encoder_position_embedding`` with every argument given: (pos [N, S, C], mask_flatten bool [N, S], valid_ratios
    float32 [N, L, 2])."""
    return _P._encoder(masks, level_embed, temporal_embed, num_pos_feats, temperature, normalize, scale, round_dtype, out_dtype)


@encoder_position_embedding_op.register_fake
def _(masks, level_embed, temporal_embed, num_pos_feats, temperature, normalize, scale, round_dtype, out_dtype):
    N, sizes, C, _, _, out_dtype = _P.check_encoder(masks, level_embed, temporal_embed, num_pos_feats, normalize, scale,
                                                    round_dtype, out_dtype)
    S = sum(h * w for h, w in sizes)
    return (_empty(level_embed, (N, S, C), out_dtype), _empty(level_embed, (N, S), torch.bool),
            _empty(level_embed, (N, len(sizes), 2), torch.float32))


@_op("encoder_position_embedding_backward")
def encoder_position_embedding_backward(grad_pos: Tensor, heights: List[int], widths: List[int], want_level: bool,
                                        want_temporal: bool) -> tuple[Tensor, Tensor]:
    """(grad_level_embed float32 [L, C], grad_temporal_embed float32 [N, C]); the one that is not wanted is empty."""
    return _P._encoder_backward(grad_pos, heights, widths, want_level, want_temporal)


@encoder_position_embedding_backward.register_fake
def _(grad_pos, heights, widths, want_level, want_temporal):
    N, _, C = grad_pos.shape
    return (_empty(grad_pos, (len(heights), C) if want_level else (0,), torch.float32),
            _empty(grad_pos, (N, C) if want_temporal else (0,), torch.float32))


encoder_position_embedding_op.register_autograd(functools.partial(_P.backward, encoder_position_embedding_backward),
                                                setup_context=_P.setup_context)


def encoder_position_embedding(masks, level_embed, temporal_embed=None, *, num_pos_feats=None, temperature=10000,
                               normalize=True, scale=None, round_dtype=None, out_dtype=None):
    """The encoder's positional input from the padding masks of all levels, on the HIP kernels of include/posembed.h: what
    DeVIS's position encoding, the ``.to(dtype)`` of its callers and ``DeformableTransformer.prepare_data`` make of them::

        pos_l        = PositionEmbeddingSine(num_pos_feats, temperature, normalize, scale)(masks[l])    # [N, C, H_l, W_l]
        pos_l        = (pos_l + temporal_embed[:, :, None, None]).to(round_dtype)                       # each where given
        pos          = cat_l(pos_l.flatten(2).transpose(1, 2) + level_embed[l], 1)                      # [N, S, C]
        mask_flatten = cat_l(masks[l].flatten(1), 1);   valid_ratios = stack_l(get_valid_ratio(masks[l]), 1)

    ``masks``: a list of bool [N, H_l, W_l] with any strides; ``level_embed`` [L, C] and ``temporal_embed`` [N, C] or None,
    in any floating dtype (the kernels read them as float32); ``num_pos_feats`` defaults to ``C // 2`` and must be even;
    ``scale`` (default ``2 * pi``) needs ``normalize``.  Arithmetic is float32 with the reference's operations in the
    reference's order.  ``round_dtype`` (bfloat16 / float16) rounds ``sine + temporal`` before the level embedding is added,
    as ``.to(dtype)`` does in the reference; ``out_dtype`` defaults to what torch's promotion gives the reference
    (``promote_types(round_dtype or float32, level_embed.dtype)``) and is rounded once at the store.

    Returns ``(pos [N, S, C], mask_flatten bool [N, S], valid_ratios float32 [N, L, 2])``.  Only ``pos`` is differentiable,
    with respect to ``level_embed`` and ``temporal_embed``: their gradients are segmented column sums of ``grad_pos`` in a
    fixed order, without atomics -- bitwise reproducible --, and only the ones autograd asks for are computed.  Two launches
    forward, two backward.  GPU tensors only."""
    masks = list(masks)
    if torch.compiler.is_compiling():
        return encoder_position_embedding_op(masks, level_embed, temporal_embed, num_pos_feats, float(temperature),
                                             bool(normalize), scale, round_dtype, out_dtype)
    return _P.EncoderPositionEmbeddingFunction.apply(level_embed, temporal_embed, num_pos_feats, float(temperature),
                                                     bool(normalize), scale, round_dtype, out_dtype, *masks)

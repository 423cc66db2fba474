"""Host checks the operator modules of the mask path share (deform_conv, attention_maps, mask_head_stage, mask_losses, mask_iou, mask_rle, mask_binary_iou, box_matching, assignment, label_loss, position_embedding, add_norm, self_attention, window_attention, pre_norm, frozen_norm, swin_ends)."""
import functools

import torch
from torch.autograd.function import once_differentiable


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


# ---- one autograd formula per operator --------------------------------------------------------------------------------------
# An operator's module states its formula once: ``setup_context(ctx, inputs, output)`` and ``backward(run, ctx, *grads)``, where
# ``run`` computes the gradients -- the host function for the eager Function (``eager_backward``), the backward custom op for
# the op's ``register_autograd`` (devis_amd/ops.py; ``op_runner`` where the op returns several gradients).  A gradient that is
# not computed is None from the host code and, since a custom op returns tensors, a 0-element tensor from an op.

def fill_slots(outputs, fakes):
    """For a custom op's result: the None of a gradient that was not computed becomes its 0-element stand-in."""
    return tuple(fake if t is None else t for t, fake in zip(outputs, fakes))


def none_slot(t):
    return t if t is not None and t.numel() else None


def none_slots(outputs):
    """Inverse of fill_slots: 0-element gradient tensors -> None."""
    return tuple(none_slot(t) for t in outputs)


def op_runner(op):
    """``op`` -- a backward custom op that returns several gradients -- as the ``run`` of a formula."""
    return lambda *args: none_slots(op(*args))


def eager_backward(formula, run, **kwargs):
    """``formula(run, ctx, *grads)`` as the ``backward`` of an eager autograd Function; a second derivative raises."""
    return staticmethod(once_differentiable(functools.partial(formula, run, **kwargs)))


def _check_device(op, named):
    """Every tensor of ``named`` -- (name, tensor or None) pairs of operator ``op`` -- is on the GPU of the first one."""
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise RuntimeError("Not implemented on the CPU (%s is not a GPU tensor)" % name)
    first, dev = named[0][0], named[0][1].device
    for name, t in named:
        _require(t is None or t.device == dev, "%s: %s is on another device than %s" % (op, name, first))


def _workspace(binding, code, shape, device):
    """An uninitialised workspace of ``binding.workspace_bytes(code, shape)`` bytes."""
    return torch.empty(binding.workspace_bytes(code, shape), dtype=torch.uint8, device=device)

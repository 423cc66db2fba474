"""Host checks the operator modules of the mask path share (deform_conv, attention_maps, mask_head_stage, mask_losses, mask_iou, mask_rle, mask_binary_iou, box_matching, assignment, label_loss, position_embedding)."""
import torch


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


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

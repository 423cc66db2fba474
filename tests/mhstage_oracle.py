"""The mask-head stage of include/mhstage.h in plain PyTorch, float64 on the CPU: test infrastructure only.

    z   = group_norm(x)                      y = relu(z)
    out = cat([interpolate(y, (H, W), "nearest") + skip[skip_index], extra], 1)

``gate`` (a bool tensor of x's shape) replaces the ReLU by ``z * gate``: the gradient comparisons give the oracle the gate
of the device for the few elements whose pre-activation is within rounding of zero."""
import torch
import torch.nn.functional as F


def pre_activation(x, num_groups, weight, bias, eps=1e-5):
    return F.group_norm(x.double(), num_groups, weight.double(), bias.double(), eps)


def mask_head_stage(x, num_groups, weight, bias, eps=1e-5, skip=None, skip_index=None, extra=None, gate=None):
    z = pre_activation(x, num_groups, weight, bias, eps)
    y = F.relu(z) if gate is None else z * gate.to(z.dtype)
    size = tuple(skip.shape[-2:]) if skip is not None else tuple(extra.shape[-2:]) if extra is not None else tuple(x.shape[-2:])
    if size != tuple(x.shape[-2:]):
        y = F.interpolate(y, size=size, mode="nearest")
    if skip is not None:
        skip = skip.double()
        y = y + (skip if skip_index is None else skip[skip_index.long()])
    return y if extra is None else torch.cat([y, extra.double()], 1)


def with_grads(x, num_groups, weight, bias, grad_out, eps=1e-5, skip=None, skip_index=None, extra=None, gate=None):
    """(out, {name: gradient}) for x, weight, bias and, where given, skip and extra; everything float64."""
    leaves = {"x": x, "weight": weight, "bias": bias, "skip": skip, "extra": extra}
    leaves = {k: v.double().detach().clone().requires_grad_(True) for k, v in leaves.items() if v is not None}
    out = mask_head_stage(leaves["x"], num_groups, leaves["weight"], leaves["bias"], eps, leaves.get("skip"), skip_index,
                          leaves.get("extra"), gate)
    grads = torch.autograd.grad(out, list(leaves.values()), grad_out.double())
    return out.detach(), dict(zip(leaves, grads))


def device_gate(z64, device_out, rel):
    """The gate the gradient tests hand the oracle: z64 > 0, except where |z64| <= rel * max|z64|, which take the device's
    (device_out > 0, from a plain float32-out call on the same x).  Returns (gate, number of such elements)."""
    near = z64.abs() <= rel * z64.abs().max()
    return torch.where(near, device_out.cpu() > 0, z64 > 0), int(near.sum())


def module_forward(state, features, bbox_mask, expand, multi_scale=True):
    """The reference MaskHeadConv's forward with plain convolutions, from a state dict: lay1, gn1, lay2, gn2, then per
    further feature adapter, merge, lay, gn; out_lay if present."""
    conv = lambda name, t, pad: F.conv2d(t, state[name + ".weight"], state[name + ".bias"], padding=pad)      # noqa: E731
    gn = lambda name, t: F.relu(F.group_norm(t, 8, state[name + ".weight"], state[name + ".bias"]))      # noqa: E731
    x = torch.cat([expand(features[0]), bbox_mask[0]], 1)
    x = gn("gn1", conv("lay1", x, 1))
    x = gn("gn2", conv("lay2", x, 1))
    for lvl, feature in enumerate(features[1:]):
        cur = expand(conv("adapter%d" % (lvl + 1), feature, 0))
        x = cur + F.interpolate(x, size=cur.shape[-2:], mode="nearest")
        if multi_scale and lvl + 1 < len(bbox_mask):
            x = torch.cat([x, bbox_mask[lvl + 1]], 1)
        x = gn("gn%d" % (lvl + 3), conv("lay%d" % (lvl + 3), x, 1))
    return conv("out_lay", x, 1) if "out_lay.weight" in state else x

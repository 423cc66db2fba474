"""Oracle of the mask head's attention maps (include/attmap.h): the formula in plain PyTorch -- float64 on the CPU for
whatever it is given as float64 -- with gradients by autograd.  ``MultiScaleMHAttentionMap`` spells the module around it
with the reference's parameter layout (projections as matrix products)."""
import torch


def attention_maps(q, k, mask=None, num_heads=8, scale=None):
    """q [B, Q, n*c], k [B, n*c, H, W], mask [B, H, W] bool or None -> [B, Q, n, H, W]:
    logit = scale * sum_c q * k (-inf where masked); out = exp(logit - max of the row) / sum of the row, a row being all
    heads and pixels of one (b, q)."""
    B, Q, D = q.shape
    c = D // num_heads
    H, W = k.shape[-2:]
    scale = float(c) ** -0.5 if scale is None else scale
    logit = scale * torch.einsum("bqnc,bnchw->bqnhw", q.view(B, Q, num_heads, c), k.view(B, num_heads, c, H, W))
    if mask is not None:
        logit = logit.masked_fill(mask.bool()[:, None, None], float("-inf"))
    flat = logit.flatten(2)
    e = torch.exp(flat - flat.max(dim=-1, keepdim=True).values)
    return (e / e.sum(dim=-1, keepdim=True)).view_as(logit)


def attention_maps_with_grads(q, k, mask, num_heads, grad_out, scale=None):
    """(out, grad_q, grad_k) in float64 for float64 copies of the operands."""
    q = q.detach().double().cpu().requires_grad_(True)
    k = k.detach().double().cpu().requires_grad_(True)
    out = attention_maps(q, k, None if mask is None else mask.cpu(), num_heads, scale)
    grad_q, grad_k = torch.autograd.grad(out, (q, k), grad_out.detach().double().cpu())
    return out.detach(), grad_q, grad_k


def module_forward(state, q, ks, masks, num_heads):
    """The module of the reference from a state dict (q_linear*, k_linear*): a list of per-level maps."""
    outs = []
    for i, k in enumerate(ks):
        sfx = "" if i == 0 else "_%d" % i
        wq, wk = state["q_linear%s.weight" % sfx], state["k_linear%s.weight" % sfx]
        bq, bk = state.get("q_linear%s.bias" % sfx), state.get("k_linear%s.bias" % sfx)
        ql = q @ wq.t() + (0 if bq is None else bq)
        kl = torch.einsum("oc,bchw->bohw", wk, k) + (0 if bk is None else bk[None, :, None, None])
        outs.append(attention_maps(ql, kl, None if masks is None else masks[i], num_heads))
    return outs

"""Stale memory for the operators' host code: ``install(monkeypatch, modules)`` replaces the name ``torch`` in those modules by
a shim whose ``empty`` and ``empty_like`` hand out what the caching allocator hands out in training -- memory that holds
whatever was there before -- in its worst form, with a guard zone on either side:

    | 0x7f bytes (at least GUARD) | payload, on a 256-byte boundary | 0x7f bytes (at least GUARD) |

The payload of a floating tensor holds the NaN bit pattern of test_unaligned_gpu._CANARY, that of an integer, bool or uint8
tensor 0x7f bytes (a bool payload is written through its uint8 view).  Shape, strides and dtype are those ``torch.empty``
would give, memory formats included (they are taken from the same call on the meta device).  Every buffer is recorded:
``guards_intact()`` says whether all guard bytes still hold 0x7f.  An element a kernel skips then shows as a NaN or as 0x7f
bytes in the result, a workspace record read before it is written poisons what is computed from it, and a store just outside
a tensor shows in a guard.  ``torch.zeros`` and everything else pass through."""
import torch

from test_unaligned_gpu import _CANARY

GUARD = 256
ALIGN = 256
FILL = 0x7f


def poison(t):
    """Fills a dense tensor with the stale pattern of its dtype."""
    if t.numel() == 0:
        return t
    if t.is_floating_point():
        bits, value = _CANARY[t.dtype]
        t.view(bits).fill_(value)
    else:
        t.view(torch.uint8).fill_(FILL)
    return t


class StaleMemory:
    """The shim: attribute access falls through to ``torch`` except for ``empty`` and ``empty_like``."""

    def __init__(self):
        self.buffers = []           # (the whole uint8 buffer, offset of the payload, bytes of the payload)

    def __getattr__(self, name):
        return getattr(torch, name)

    def _allocate(self, meta, device, requires_grad=False):
        assert meta.layout == torch.strided and (meta.dtype in _CANARY or not meta.is_floating_point()), meta.dtype
        nbytes = meta.numel() * meta.element_size()
        # (torch.empty and torch.empty_like only ever give dense tensors: the elements fill the storage exactly)
        assert meta.numel() == 0 or 1 + sum((n - 1) * s for n, s in zip(meta.shape, meta.stride())) == meta.numel()
        whole = torch.full((GUARD + ALIGN + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        at = GUARD + (-(whole.data_ptr() + GUARD)) % ALIGN
        payload = whole[at:at + nbytes].view(meta.dtype)
        assert payload.numel() == 0 or payload.data_ptr() % ALIGN == 0
        poison(payload)
        self.buffers.append((whole, at, nbytes))
        out = payload.as_strided(tuple(meta.shape), tuple(meta.stride()))
        return out.requires_grad_() if requires_grad else out

    def empty(self, *size, dtype=None, device=None, requires_grad=False, **kw):
        assert "out" not in kw
        meta = torch.empty(*size, dtype=dtype, device="meta", **kw)
        return self._allocate(meta, torch.device("cpu") if device is None else device, requires_grad)

    def empty_like(self, like, *, dtype=None, device=None, requires_grad=False, **kw):
        src = torch.empty_strided(like.shape, like.stride(), dtype=like.dtype, device="meta")
        meta = torch.empty_like(src, dtype=dtype, **kw)
        return self._allocate(meta, like.device if device is None else device, requires_grad)

    def guards_intact(self):
        """Whether the bytes before and after every payload handed out so far still hold 0x7f (after a synchronize)."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return all(bool((whole[:at] == FILL).all()) and bool((whole[at + nbytes:] == FILL).all())
                   for whole, at, nbytes in self.buffers)


def install(monkeypatch, modules):
    """Replaces ``torch`` in every module of ``modules`` (each must have imported it under that name) for the duration of
    the test; returns the shim."""
    shim = StaleMemory()
    for module in modules:
        assert getattr(module, "torch", None) is torch, module.__name__
        monkeypatch.setattr(module, "torch", shim)
    return shim

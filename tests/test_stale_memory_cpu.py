"""CPU tests of tests/stale_memory.py, the shim the stale-memory GPU tests put in the place of ``torch`` in the operators'
host code: what it hands out is poisoned, has the shape, strides and dtype of ``torch.empty``'s, starts on a 256-byte boundary
between two guard zones, and a write into a guard is noticed."""
import types

import pytest
import torch

import stale_memory

FLOATS = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
OTHERS = [torch.int32, torch.int64, torch.uint8, torch.bool]


def raw_bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize("dtype", FLOATS + OTHERS, ids=lambda d: str(d).split(".")[1])
def test_the_payload_is_poisoned_and_lies_aligned_between_two_guards(dtype):
    shim = stale_memory.StaleMemory()
    t = shim.empty((3, 5), dtype=dtype)
    assert t.dtype == dtype and tuple(t.shape) == (3, 5) and t.is_contiguous() and t.data_ptr() % 256 == 0
    if dtype in FLOATS:
        assert bool(torch.isnan(t).all())
    else:
        assert bool((raw_bytes(t) == 0x7f).all())
    (whole, at, nbytes), = shim.buffers
    assert nbytes == 15 * t.element_size() and at >= 256 and whole.numel() - at - nbytes >= 256
    assert whole[at:].data_ptr() == t.data_ptr() and whole.dtype == torch.uint8
    assert bool((whole[:at] == 0x7f).all()) and bool((whole[at + nbytes:] == 0x7f).all()) and shim.guards_intact()


def test_shapes_strides_and_dtypes_are_those_of_torch_empty():
    shim = stale_memory.StaleMemory()
    like = torch.zeros(2, 6, 4, 5)
    last = like.contiguous(memory_format=torch.channels_last)
    permuted = like.permute(0, 2, 3, 1)
    calls = [
        ("empty", ((4, 3, 2),), dict(dtype=torch.float32)),
        ("empty", (4, 3, 2), dict(dtype=torch.int64)),
        ("empty", (6,), dict(dtype=torch.uint8)),
        ("empty", ((),), dict(dtype=torch.float64)),
        ("empty", ((0,),), dict(dtype=torch.float32)),
        ("empty", ((2, 0, 3),), dict(dtype=torch.int32)),
        ("empty", ((2, 6, 4, 5),), dict(dtype=torch.bfloat16, memory_format=torch.channels_last)),
        ("empty", ((2, 1, 4, 5),), dict(dtype=torch.float32, memory_format=torch.channels_last)),
        ("empty", (torch.Size([3, 7]),), dict(dtype=torch.bool)),
        ("empty_like", (like,), {}),
        ("empty_like", (last,), {}),
        ("empty_like", (permuted,), {}),
        ("empty_like", (last,), dict(memory_format=torch.contiguous_format)),
        ("empty_like", (like,), dict(memory_format=torch.channels_last)),
        ("empty_like", (permuted,), dict(dtype=torch.float16)),
        ("empty_like", (like[:, ::2],), {}),                        # not dense: torch.empty_like makes it dense
    ]
    for name, args, kw in calls:
        got, want = getattr(shim, name)(*args, **kw), getattr(torch, name)(*args, **kw)
        assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride(), (name, args, kw)
        assert got.device == want.device and not got.requires_grad
        assert got.numel() == 0 or got.data_ptr() % 256 == 0
        if got.is_floating_point() and got.numel():
            assert bool(torch.isnan(got).all())
    assert len(shim.buffers) == len(calls) and shim.guards_intact()
    assert shim.empty((2,), dtype=torch.float32, requires_grad=True).requires_grad
    # the rest of torch passes through
    assert shim.zeros is torch.zeros and shim.float32 is torch.float32 and shim.autograd is torch.autograd


def test_writing_the_payload_leaves_the_guards_and_writing_a_guard_is_noticed():
    for where in ("before", "after"):
        shim = stale_memory.StaleMemory()
        a, b = shim.empty((5, 3), dtype=torch.float32), shim.empty(11, dtype=torch.uint8)
        a.fill_(1.0)
        b.fill_(0)
        assert shim.guards_intact() and float(a.sum()) == 15.0
        whole, at, nbytes = shim.buffers[1]
        whole[at - 1 if where == "before" else at + nbytes] = 0            # one byte just outside the second payload
        assert not shim.guards_intact(), where


def test_install_replaces_torch_in_the_given_modules_until_the_test_ends():
    module = types.ModuleType("stand_in")
    module.torch = torch
    module.make = lambda: (module.torch.empty((4,), dtype=module.torch.float32), module.torch.zeros(2))       # noqa: E731
    with pytest.MonkeyPatch.context() as patch:
        shim = stale_memory.install(patch, [module])
        assert module.torch is shim
        stale, zeros = module.make()
        assert bool(torch.isnan(stale).all()) and zeros.tolist() == [0.0, 0.0] and len(shim.buffers) == 1
    assert module.torch is torch
    with pytest.raises(AssertionError):              # a module that does not allocate through the name `torch` is an error
        stale_memory.install(pytest.MonkeyPatch(), [types.ModuleType("nothing")])

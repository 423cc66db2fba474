"""CPU tests of the opt-in order-independent grad_input of the deformable convolution: the two new entry points of
include/mdcn.h (exports, version, workspace arithmetic, argument errors -- no compute calls), the switch
``devis_amd.reproducible_grad_input`` in its three forms, how a layer's override reaches the backward, the determinism
check with the switch on and off, and the fake-tensor path.  The kernels are tests/test_dcn_reproducible_gpu.py."""
import ctypes
import os
import re
import types
import warnings

import pytest
import torch

from conftest import ROOT


def _shape(**kw):
    from devis_amd import _mdcn
    d = dict(N=1, C=8, H=6, W=7, Ho=6, Wo=7, Kh=3, Kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, G=2)
    d.update(kw)
    return _mdcn.Shape(**d)


@pytest.fixture
def switch_off():
    """Every test starts with the switch off and leaves it as it found it."""
    from devis_amd.functions import deform_conv as D
    was = D.reproducible_grad_input_enabled()
    D.reproducible_grad_input(False)
    try:
        yield
    finally:
        D.reproducible_grad_input(was)


# ---- library ---------------------------------------------------------------------------------------------------------

def test_the_two_new_symbols_are_exported_and_the_abi_is_version_2():
    from devis_amd import _mdcn, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "mdcn.h")).read()
    raw = ctypes.CDLL(path)
    for name in ("mdcn_fixed_workspace_bytes", "mdcn_backward_input_fixed"):
        assert name in _mdcn.EXPORTED_SYMBOLS and hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    lib = _mdcn.load()
    assert lib.mdcn_version() == _mdcn.MDCN_ABI_VERSION == 2
    assert int(re.search(r"#define MDCN_ABI_VERSION (\d+)", header).group(1)) == 2
    assert lib.msda_build_info().decode() == "abi=14 arch=gfx950"


def _r256(v):
    return (v + 255) // 256 * 256


def test_fixed_workspace_bytes_is_the_documented_arithmetic():
    from devis_amd import _mdcn
    lib = _mdcn.load()
    ok = _shape()
    # 3 images of 6 x 7 x 8: 1008 elements -> 8064 B of int64 (-> 8192), 126 words of nibbles = 504 B (-> 512), 48 B of maxima (-> 256)
    assert lib.mdcn_fixed_workspace_bytes(0, ctypes.byref(ok), 3) == 8192 + 512 + 256 == 8960
    for code in range(6):       # the accumulators are int64 whatever the storage type
        assert lib.mdcn_fixed_workspace_bytes(code, ctypes.byref(ok), 3) == 8960
    # an element count that is not a multiple of 8: 5 * 3 * 3 = 45 elements, 6 nibble words
    odd = _shape(C=3, H=5, W=3, Ho=5, Wo=3, G=1)
    assert lib.mdcn_fixed_workspace_bytes(1, ctypes.byref(odd), 1) == _r256(45 * 8) + _r256(6 * 4) + _r256(16) == 512 + 256 + 256
    elems = 60 * 90 * 160 * 32
    big = _shape(C=32, H=90, W=160, Ho=90, Wo=160, G=1)
    assert _mdcn.fixed_workspace_bytes(2, big, 60) == _r256(elems * 8) + _r256(elems // 8 * 4) + _r256(60 * 16)
    assert lib.mdcn_fixed_workspace_bytes(0, ctypes.byref(ok), 0) == 0
    assert _mdcn.fixed_workspace_bytes(0, _shape(N=77), 3) == 8960                   # shape.N is ignored
    assert lib.mdcn_fixed_workspace_bytes(0, ctypes.byref(ok), -1) == -1 and b"positive" in lib.mdcn_last_error()
    assert lib.mdcn_fixed_workspace_bytes(9, ctypes.byref(ok), 1) == -1 and b"dtype" in lib.mdcn_last_error()
    assert lib.mdcn_fixed_workspace_bytes(0, None, 1) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert lib.mdcn_fixed_workspace_bytes(0, ctypes.byref(_shape(Ho=5)), 1) == -1 and b"output size" in lib.mdcn_last_error()
    with pytest.raises(RuntimeError, match="multiple"):
        _mdcn.fixed_workspace_bytes(0, _shape(G=3), 1)


def test_backward_input_fixed_argument_errors_without_gpu():
    from devis_amd import _mdcn
    lib = _mdcn.load()
    buf = ctypes.create_string_buffer(1024)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 255) // 256 * 256)
    ok = _shape()
    call = lib.mdcn_backward_input_fixed
    assert call(0, None, p, p, ctypes.byref(ok), p, p, None) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert call(0, p, p, None, ctypes.byref(ok), p, p, None) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert call(0, p, p, p, ctypes.byref(ok), None, p, None) == -1 and b"workspace" in lib.mdcn_last_error()
    assert call(0, p, p, p, ctypes.byref(ok), p, None, None) == -1 and b"grad_input" in lib.mdcn_last_error()
    assert call(0, p, p, p, None, p, p, None) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert call(0, p, p, p, ctypes.byref(ok), ctypes.c_void_p(p.value + 8), p, None) == -1 and b"aligned" in lib.mdcn_last_error()
    assert call(9, p, p, p, ctypes.byref(ok), p, p, None) == -1 and b"dtype" in lib.mdcn_last_error()
    assert call(0, p, p, p, ctypes.byref(_shape(G=3)), p, p, None) == -1 and b"multiple" in lib.mdcn_last_error()
    assert call(0, p, p, p, ctypes.byref(_shape(N=-1)), p, p, None) == -1 and b"positive" in lib.mdcn_last_error()
    assert call(0, p, p, p, ctypes.byref(_shape(Ho=5)), p, p, None) == -1 and b"output size" in lib.mdcn_last_error()
    assert call(0, p, None, p, ctypes.byref(_shape(N=0)), p, p, None) == 0      # empty batch: no-op, nothing launched
    # mdcn_backward is as it was: a third gradient group does not exist
    assert lib.mdcn_backward(8, 0, p, p, p, p, ctypes.byref(ok), p, p, p, None) == -1 and b"grads" in lib.mdcn_last_error()
    assert lib.mdcn_backward(4, 0, p, p, p, p, ctypes.byref(ok), p, p, p, None) == -1 and b"grads" in lib.mdcn_last_error()


# ---- the switch ------------------------------------------------------------------------------------------------------

def test_switch_as_a_call_as_a_context_manager_nested_and_after_an_exception(switch_off):
    import devis_amd
    from devis_amd.functions import deform_conv as D
    assert devis_amd.reproducible_grad_input is D.reproducible_grad_input
    assert devis_amd.reproducible_grad_input_enabled is D.reproducible_grad_input_enabled
    assert "reproducible_grad_input" in devis_amd.__all__ and "reproducible_grad_input_enabled" in devis_amd.__all__
    on = devis_amd.reproducible_grad_input_enabled
    assert on() is False
    devis_amd.reproducible_grad_input()                 # a plain call: the process-wide default
    assert on() is True
    devis_amd.reproducible_grad_input(False)
    assert on() is False
    with devis_amd.reproducible_grad_input():
        assert on() is True
        with devis_amd.reproducible_grad_input(False):
            assert on() is False
            with devis_amd.reproducible_grad_input(True):
                assert on() is True
            assert on() is False
        assert on() is True
    assert on() is False
    with pytest.raises(ZeroDivisionError):
        with devis_amd.reproducible_grad_input():
            assert on() is True
            1 / 0
    assert on() is False
    devis_amd.reproducible_grad_input(True)
    with devis_amd.reproducible_grad_input(False):
        assert on() is False
    assert on() is True                                 # a context manager restores what it found, not "off"


def test_what_is_pinned_for_a_call_overrides_the_switch_both_ways(switch_off):
    from devis_amd.functions import deform_conv as D
    assert D.NEED_ALL == 31 and D.PIN_FIXED & D.NEED_ALL == 0 and D.PIN_FLOAT & D.NEED_ALL == 0
    assert (D.pin_bits(None), D.pin_bits(True), D.pin_bits(False)) == (0, D.PIN_FIXED, D.PIN_FLOAT)
    assert D.input_mode(D.NEED_ALL) == (31, False)
    assert D.input_mode(D.NEED_ALL | D.PIN_FIXED) == (31, True)
    assert D.input_mode(D.NEED_INPUT | D.PIN_FLOAT) == (1, False)
    assert D.input_mode((D.NEED_ALL & ~D.NEED_INPUT) | D.PIN_FIXED) == (30, False)      # no grad_input: nothing to fix
    with D.reproducible_grad_input():
        assert D.input_mode(D.NEED_ALL) == (31, True)
        assert D.input_mode(D.NEED_ALL | D.PIN_FLOAT) == (31, False)
        assert D.input_mode(D.NEED_ALL | D.PIN_FIXED) == (31, True)
        assert D.input_mode(D.NEED_WEIGHT) == (8, False)
    with pytest.raises(RuntimeError, match="pins"):
        D.input_mode(D.NEED_ALL | D.PIN_FIXED | D.PIN_FLOAT)


def _args(N=2, C=4, H=5, W=6, Co=3, K=3, dtype=torch.float32, device="cpu"):
    x = torch.zeros(N, C, H, W, dtype=dtype, device=device)
    off = torch.zeros(N, 2 * K * K, H, W, dtype=dtype, device=device)
    w = torch.zeros(Co, C, K, K, dtype=dtype, device=device)
    return x, off, w, torch.zeros(N, K * K, H, W, dtype=dtype, device=device)


def test_the_module_attribute_reaches_the_backward_op_as_a_pin_bit(monkeypatch, switch_off):
    """The layer's override travels forward op -> setup_context -> `grads` of the 9-argument backward op; None adds no bit."""
    from devis_amd import ops
    from devis_amd.functions import deform_conv as D
    from devis_amd.functions._common import op_runner
    from devis_amd.modules import ModulatedDeformableConv2d
    seen = []

    def fake_backward(grad_out, input, offset, weight, mask, stride, padding, dilation, grads):
        seen.append(grads)
        return (torch.zeros_like(input), torch.zeros_like(offset), torch.zeros_like(mask), torch.zeros_like(weight),
                torch.zeros(weight.shape[0]))

    monkeypatch.setattr(ops, "deform_conv2d_backward", fake_backward)
    x, off, w, m = _args()
    for pinned, want in ((None, 31), (True, 31 | D.PIN_FIXED), (False, 31 | D.PIN_FLOAT)):
        ctx = types.SimpleNamespace(needs_input_grad=(True, True, True, True, False, False, False, True))
        inputs = (x, off, w, None, [1, 1], [1, 1], [1, 1], m)
        ctx.save_for_backward = lambda *t: setattr(ctx, "saved_tensors", t)
        run = op_runner(ops.deform_conv2d_backward)
        if pinned is None:
            D.setup_context(ctx, inputs, None)
            out = D.backward(run, ctx, torch.zeros(2, 3, 5, 6))
            assert len(out) == 8
        else:
            D.setup_context(ctx, inputs + (pinned,), None)
            out = D.backward(run, ctx, torch.zeros(2, 3, 5, 6))
            assert len(out) == 9 and out[8] is None
        assert seen[-1] == want
    # the module hands its attribute to the operator; the default is None, and it is in no state dict
    calls = []
    monkeypatch.setattr(ops, "deform_conv2d", lambda *a, **kw: calls.append(kw["reproducible_grad_input"]) or a[0])
    layer = ModulatedDeformableConv2d(4, 3)
    assert layer.reproducible_grad_input is None
    for value in (None, True, False):
        layer.reproducible_grad_input = value
        layer(torch.zeros(1, 4, 5, 6))
    assert calls == [None, True, False]
    assert not any("reproducible" in k for k in layer.state_dict())
    plain = ModulatedDeformableConv2d(4, 3)
    plain.load_state_dict(layer.state_dict(), strict=True)
    layer.load_state_dict(plain.state_dict(), strict=True)
    assert layer.reproducible_grad_input is False and plain.reproducible_grad_input is None


def test_operator_keyword_picks_the_forward_op(monkeypatch, switch_off):
    import devis_amd
    from devis_amd import ops
    x, off, w, m = _args()
    seen = []
    monkeypatch.setattr(ops, "deform_conv2d_op", lambda *a: seen.append(("plain", len(a), None)) or a[0])
    monkeypatch.setattr(ops, "deform_conv2d_pinned_op", lambda *a: seen.append(("pinned", len(a), a[8])) or a[0])
    for value in (None, True, False, 1):
        devis_amd.deform_conv2d(x, off, w, None, 1, 1, 1, m, reproducible_grad_input=value)
    devis_amd.deform_conv2d(x, off, w, None, 1, 1, 1, m)
    assert seen == [("plain", 8, None), ("pinned", 9, True), ("pinned", 9, False), ("pinned", 9, True), ("plain", 8, None)]
    monkeypatch.undo()
    for value in (None, True, False):       # unpatched, all three reach the host code, which refuses CPU tensors
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            devis_amd.deform_conv2d(x, off, w, None, 1, 1, 1, m, reproducible_grad_input=value)


# ---- determinism check -----------------------------------------------------------------------------------------------

PINNED = "deform_conv2d_backward does not have a deterministic implementation"


def test_with_the_switch_on_the_backward_gets_past_the_determinism_check_without_a_warning(switch_off):
    from devis_amd.functions import deform_conv as D
    x, off, w, m = _args()
    call = lambda grads: D._backward(torch.zeros(2, 3, 5, 6), x, off, w, m, (1, 1), (1, 1), (1, 1), grads)    # noqa: E731
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        for warn_only in (False, True):
            torch.use_deterministic_algorithms(True, warn_only=warn_only)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                with D.reproducible_grad_input():
                    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                        call(D.NEED_ALL)
                    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                        call(D.NEED_INPUT)
                with pytest.raises(RuntimeError, match="Not implemented on the CPU"):       # pinned for the call, switch off
                    call(D.NEED_ALL | D.PIN_FIXED)
        # pinned to float atomics under the switch: the check is back
        torch.use_deterministic_algorithms(True)
        with D.reproducible_grad_input():
            with pytest.raises(RuntimeError, match=PINNED):
                call(D.NEED_ALL | D.PIN_FLOAT)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)


def test_with_the_switch_off_the_message_keeps_its_pinned_words_and_names_the_switch(switch_off):
    from devis_amd.functions import deform_conv as D
    x, off, w, m = _args()
    call = lambda grads: D._backward(torch.zeros(2, 3, 5, 6), x, off, w, m, (1, 1), (1, 1), (1, 1), grads)    # noqa: E731
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError) as err:
            call(D.NEED_ALL)
        assert PINNED in str(err.value) and "devis_amd.reproducible_grad_input" in str(err.value)
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning) as seen:
            with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                call(D.NEED_INPUT)
        text = " ".join(str(w.message) for w in seen)
        assert PINNED in text and "devis_amd.reproducible_grad_input" in text
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _dcn_nodes(graph):
    return [n for n in graph.nodes if n.op == "call_function" and "deform_conv2d" in str(n.target)
            and "backward" not in str(n.target)]


@pytest.mark.parametrize("override", [True, False])
def test_export_of_the_module_with_the_override_gives_one_op_node_that_carries_it(override, switch_off):
    from devis_amd.modules import ModulatedDeformableConv2d
    m = ModulatedDeformableConv2d(8, 4, bias=True).to("meta")
    m.reproducible_grad_input = override
    ep = torch.export.export(m, (torch.empty(2, 8, 12, 20, device="meta"),))
    nodes = _dcn_nodes(ep.graph)
    assert len(nodes) == 1 and "deform_conv2d_pinned" in str(nodes[0].target)
    assert nodes[0].args[-1] is override
    assert tuple(nodes[0].meta["val"].shape) == (2, 4, 12, 20)


def test_the_backward_op_accepts_the_pin_bits_on_fake_tensors_and_nothing_beyond_them():
    from devis_amd import ops
    from devis_amd.functions import deform_conv as D
    x, off, w, m = _args(device="meta")
    g = torch.empty(2, 3, 5, 6, device="meta")
    for grads in (D.NEED_ALL, D.NEED_ALL | D.PIN_FIXED, D.NEED_INPUT | D.PIN_FLOAT):
        out = ops._fake_deform_conv2d_backward(g, x, off, w, m, [1, 1], [1, 1], [1, 1], grads)
        assert out[0].shape == x.shape
    with pytest.raises(RuntimeError, match="NEED_"):
        ops._fake_deform_conv2d_backward(g, x, off, w, m, [1, 1], [1, 1], [1, 1], 128)

"""CPU tests of the modulated deformable convolution: the oracle against F.conv2d, the C ABI of include/mdcn.h (exports,
version, argument errors -- no compute calls), the host code (shape checks, errors, deterministic mode, gradient masks),
the module and patch_mask_head, and the fake-tensor paths.  The kernels themselves are tests/test_dcn_gpu.py."""
import ctypes
import os
import re
import types
import warnings

import pytest
import torch
import torch.nn.functional as F

import dcn_oracle
from conftest import ROOT


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


# ---- oracle self-checks ----------------------------------------------------------------------------------------------

CONV_CASES = [  # (H, W, Kh, Kw, stride, padding, dilation)
    (7, 9, 3, 3, (1, 1), (1, 1), (1, 1)),
    (8, 11, 3, 2, (2, 1), (2, 0), (1, 2)),
    (9, 6, 1, 1, (2, 2), (0, 0), (1, 1)),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_oracle_with_zero_offsets_is_a_convolution(case):
    H, W, Kh, Kw, stride, padding, dilation = case
    x, w, b = _rand(2, 4, H, W), _rand(3, 4, Kh, Kw, seed=1), _rand(3, seed=2)
    ref = F.conv2d(x, w, b, stride, padding, dilation)
    off = torch.zeros(2, 2 * 2 * Kh * Kw, ref.shape[2], ref.shape[3], dtype=torch.float64)     # two offset groups
    assert torch.equal(dcn_oracle.deform_conv2d(x, off, w, b, stride, padding, dilation), ref) or \
        float((dcn_oracle.deform_conv2d(x, off, w, b, stride, padding, dilation) - ref).abs().max()) <= 1e-13


@pytest.mark.parametrize("shift", [(1, -2), (-3, 0), (0, 4)])
def test_oracle_with_an_integer_offset_is_a_convolution_of_the_translated_zero_extended_input(shift):
    dy, dx = shift
    x, w = _rand(2, 3, 6, 8), _rand(4, 3, 3, 3, seed=1)
    P = 6                                                   # zero margin wider than any shift + the kernel
    big = F.pad(x, (P, P, P, P))
    ref = F.conv2d(big, w)[:, :, P - 1 + dy:P - 1 + dy + 6, P - 1 + dx:P - 1 + dx + 8]      # padding=1 output, read at (+dy, +dx)
    off = torch.zeros(2, 18, 6, 8, dtype=torch.float64)
    off[:, 0::2], off[:, 1::2] = dy, dx
    got = dcn_oracle.deform_conv2d(x, off, w, None, 1, 1, 1)
    assert float((got - ref).abs().max()) <= 1e-13


def test_oracle_mask_of_ones_is_no_mask_and_gradcheck_passes():
    x, w, b = _rand(1, 4, 5, 6), _rand(2, 4, 3, 3, seed=1), _rand(2, seed=2)
    off = torch.rand(1, 2 * 2 * 9, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 0.8 + 0.1
    ones = torch.ones(1, 18, 5, 6, dtype=torch.float64)
    assert torch.equal(dcn_oracle.deform_conv2d(x, off, w, b, 1, 1, 1, None), dcn_oracle.deform_conv2d(x, off, w, b, 1, 1, 1, ones))
    msk = torch.rand(1, 18, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    leaves = [t.clone().requires_grad_(True) for t in (x, off, w, b, msk)]
    assert torch.autograd.gradcheck(lambda x, o, w, b, m: dcn_oracle.deform_conv2d(x, o, w, b, 1, 1, 1, m), leaves)


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_mdcn_h_declares_and_versions_agree():
    from devis_amd import _mdcn, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "mdcn.h")).read()
    declared = set(re.findall(r"\b(mdcn_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_mdcn.EXPORTED_SYMBOLS) and len(declared) >= 5
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _mdcn.load()
    assert lib.mdcn_version() == _mdcn.MDCN_ABI_VERSION == int(re.search(r"#define MDCN_ABI_VERSION (\d+)", header).group(1))
    assert (_mdcn.GRAD_INPUT, _mdcn.GRAD_SAMPLING) == tuple(
        int(re.search(r"#define MDCN_GRAD_%s (\d+)" % n, header).group(1)) for n in ("INPUT", "SAMPLING"))
    # the attention ABI is untouched
    assert lib.msda_build_info().decode() == "abi=14 arch=gfx950"
    assert os.path.join(build.include_dir(), "mdcn.h") in build._headers()


def _shape(**kw):
    from devis_amd import _mdcn
    d = dict(N=1, C=8, H=6, W=7, Ho=6, Wo=7, Kh=3, Kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, G=2)
    d.update(kw)
    return _mdcn.Shape(**d)


def test_mdcn_argument_errors_without_gpu():
    from devis_amd import _mdcn
    lib = _mdcn.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = _shape()
    assert lib.mdcn_im2col(0, None, p, p, ctypes.byref(ok), p, None) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(0, p, p, p, None, p, None) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(9, p, p, p, ctypes.byref(ok), p, None) == -1 and b"dtype" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(0, p, p, p, ctypes.byref(_shape(G=3)), p, None) == -1 and b"multiple" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(0, p, p, p, ctypes.byref(_shape(N=-1)), p, None) == -1 and b"positive" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(0, p, p, p, ctypes.byref(_shape(H=-6)), p, None) == -1 and b"positive" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(0, p, p, p, ctypes.byref(_shape(Ho=5)), p, None) == -1 and b"output size" in lib.mdcn_last_error()
    assert lib.mdcn_im2col(0, p, p, p, ctypes.byref(_shape(N=0)), p, None) == 0       # empty batch: no-op, nothing launched
    assert lib.mdcn_backward(3, 0, p, p, p, None, ctypes.byref(ok), p, p, p, None) == -1 and b"null pointer" in lib.mdcn_last_error()
    assert lib.mdcn_backward(1, 0, p, p, p, p, ctypes.byref(ok), None, None, None, None) == -1 and b"grad_input_acc" in lib.mdcn_last_error()
    assert lib.mdcn_backward(2, 0, p, p, p, p, ctypes.byref(ok), None, p, None, None) == -1 and b"grad_mask" in lib.mdcn_last_error()
    assert lib.mdcn_backward(8, 0, p, p, p, p, ctypes.byref(ok), p, p, p, None) == -1 and b"grads" in lib.mdcn_last_error()
    assert lib.mdcn_backward(0, 0, p, p, p, p, ctypes.byref(ok), None, None, None, None) == 0    # nothing asked for
    assert lib.mdcn_workspace_bytes(2, ctypes.byref(ok), 5) == 5 * 6 * 7 * 9 * 8 * 2
    assert lib.mdcn_workspace_bytes(1, ctypes.byref(ok), 1) == 6 * 7 * 9 * 8 * 8
    assert lib.mdcn_workspace_bytes(0, ctypes.byref(ok), -1) == -1
    with pytest.raises(RuntimeError, match="multiple"):
        _mdcn.workspace_bytes(0, _shape(G=3), 1)


# ---- host ------------------------------------------------------------------------------------------------------------

def _args(N=2, C=4, H=5, W=6, Co=3, K=3, G=1, dtype=torch.float32, device="cpu", mask=True, bias=True):
    x = torch.zeros(N, C, H, W, dtype=dtype, device=device)
    off = torch.zeros(N, 2 * G * K * K, H, W, dtype=dtype, device=device)
    w = torch.zeros(Co, C, K, K, dtype=dtype, device=device)
    return dict(input=x, offset=off, weight=w, bias=torch.zeros(Co, dtype=dtype, device=device) if bias else None,
                stride=1, padding=K // 2, dilation=1, mask=torch.zeros(N, G * K * K, H, W, dtype=dtype, device=device) if mask else None)


def test_operator_raises_on_cpu_tensors_and_on_bad_shapes_before_any_launch():
    import devis_amd
    from devis_amd.functions import deform_conv as D
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.deform_conv2d(**_args())
    assert devis_amd.deform_conv2d is devis_amd.ops.deform_conv2d

    def check(**changes):
        a = _args(device="meta")
        a.update(changes)
        pair = lambda v: (v, v) if isinstance(v, int) else v        # noqa: E731
        return D.check_shapes(a["input"], a["offset"], a["weight"], a["bias"], pair(a["stride"]), pair(a["padding"]),
                              pair(a["dilation"]), a["mask"])

    assert check() == (5, 6, 1)
    assert check(offset=torch.zeros(2, 36, 5, 6, device="meta"), mask=torch.zeros(2, 18, 5, 6, device="meta")) == (5, 6, 2)
    assert check(stride=(2, 1), padding=(0, 2), offset=torch.zeros(2, 18, 2, 8, device="meta"), mask=None) == (2, 8, 1)
    with pytest.raises(NotImplementedError, match="weight groups"):
        check(weight=torch.zeros(3, 2, 3, 3, device="meta"))
    with pytest.raises(RuntimeError, match="does not match"):
        check(weight=torch.zeros(3, 3, 3, 3, device="meta"))
    with pytest.raises(RuntimeError, match="offset must be"):
        check(offset=torch.zeros(2, 18, 5, 5, device="meta"))
    with pytest.raises(RuntimeError, match="multiple of 2"):
        check(offset=torch.zeros(2, 17, 5, 6, device="meta"))
    with pytest.raises(RuntimeError, match="offset groups"):
        check(offset=torch.zeros(2, 54, 5, 6, device="meta"), mask=None)       # G = 3, C = 4
    with pytest.raises(RuntimeError, match="mask must be"):
        check(mask=torch.zeros(2, 18, 5, 6, device="meta"))
    with pytest.raises(RuntimeError, match="bias must be"):
        check(bias=torch.zeros(4, device="meta"))
    with pytest.raises(RuntimeError, match="weight must have input's dtype"):
        check(weight=torch.zeros(3, 4, 3, 3, dtype=torch.float16, device="meta"))
    with pytest.raises(RuntimeError, match="float32 beside a 16-bit input"):
        check(offset=torch.zeros(2, 18, 5, 6, dtype=torch.float64, device="meta"), mask=None)
    with pytest.raises(RuntimeError, match="would be empty"):
        check(padding=0, dilation=4)
    # float32 offsets and mask beside a 16-bit input are part of the contract
    h = _args(dtype=torch.bfloat16, device="meta")
    h["offset"], h["mask"] = h["offset"].float(), h["mask"].float()
    assert D.check_shapes(h["input"], h["offset"], h["weight"], h["bias"], (1, 1), (1, 1), (1, 1), h["mask"]) == (5, 6, 1)


def test_deterministic_mode_raises_or_warns_only_when_grad_input_is_asked_for():
    from devis_amd.functions import deform_conv as D
    a = _args()
    call = lambda grads: D._backward(torch.zeros(2, 3, 5, 6), a["input"], a["offset"], a["weight"], a["mask"],   # noqa: E731
                                     (1, 1), (1, 1), (1, 1), grads)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="deform_conv2d_backward does not have a deterministic implementation"):
            call(D.NEED_ALL)
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):       # past the check: the other gradients are deterministic
            call(D.NEED_ALL & ~D.NEED_INPUT)
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match="deform_conv2d_backward does not have a deterministic implementation"):
            with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                call(D.NEED_INPUT)
        torch.use_deterministic_algorithms(False)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                call(D.NEED_ALL)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)


def test_needs_input_grad_maps_to_the_gradient_mask(monkeypatch):
    from devis_amd import ops
    from devis_amd.functions import deform_conv as D
    from devis_amd.functions._common import op_runner
    assert D.grads_mask(True, False, False, False, False) == D.NEED_INPUT == 1
    assert D.grads_mask(False, True, True, False, False) == D.NEED_OFFSET | D.NEED_MASK == 6
    assert D.grads_mask(True, True, True, True, True) == D.NEED_ALL == 31
    seen = []

    def fake_backward(grad_out, input, offset, weight, mask, stride, padding, dilation, grads):
        seen.append(grads)
        return (torch.zeros_like(input), torch.zeros_like(offset), None if mask is None else torch.zeros_like(mask),
                torch.zeros_like(weight), torch.zeros(weight.shape[0]))

    monkeypatch.setattr(ops, "deform_conv2d_backward", fake_backward)
    a = _args()
    for needs, mask, want in (((True, True, True, True, False, False, False, True), a["mask"], 31),
                              ((False, False, True, True, False, False, False, False), a["mask"], 24),
                              ((False, True, False, False, False, False, False, True), None, 2),
                              ((True, False, False, False, False, False, False, False), a["mask"], 1)):
        ctx = types.SimpleNamespace(saved_tensors=(a["input"], a["offset"], a["weight"], mask), needs_input_grad=needs,
                                    geometry=([1, 1], [1, 1], [1, 1]))
        out = D.backward(op_runner(ops.deform_conv2d_backward), ctx, torch.zeros(2, 3, 5, 6))
        assert seen[-1] == want and len(out) == 8 and out[4:7] == (None, None, None)


def test_module_state_dict_initialisation_and_reference_checkpoint():
    from devis_amd.modules import ModulatedDeformableConv2d
    m = ModulatedDeformableConv2d(8, 4, bias=True)
    assert list(m.state_dict()) == ["offset_conv.weight", "offset_conv.bias", "modulator_conv.weight", "modulator_conv.bias",
                                    "regular_conv.weight", "regular_conv.bias"]
    assert list(ModulatedDeformableConv2d(8, 4).state_dict())[-1] == "regular_conv.weight"      # bias=False is the default
    for conv in (m.offset_conv, m.modulator_conv):
        assert float(conv.weight.detach().abs().max()) == 0.0 and float(conv.bias.detach().abs().max()) == 0.0
    assert m.offset_conv.weight.shape == (18, 8, 3, 3) and m.modulator_conv.weight.shape == (9, 8, 3, 3)
    assert float(m.regular_conv.weight.detach().abs().max()) > 0
    # a state dict with the reference's keys and shapes loads strictly (the oracle module spells the reference's layout)
    ref = dcn_oracle.ModulatedDeformableConv2d(8, 4, bias=True)
    m.load_state_dict(ref.state_dict(), strict=True)
    assert torch.equal(m.offset_conv.weight, ref.offset_conv.weight)


def test_patch_mask_head_replaces_the_class_in_a_stand_in_module():
    import devis_amd
    from devis_amd import argument_builders

    class Theirs(torch.nn.Module):
        pass

    seg = types.SimpleNamespace(ModulatedDeformableConv2d=Theirs)
    previous = devis_amd.patch_mask_head(seg)
    assert previous is Theirs and seg.ModulatedDeformableConv2d is devis_amd.modules.ModulatedDeformableConv2d
    layer = seg.ModulatedDeformableConv2d(16, 1, kernel_size=3, padding=1)
    assert isinstance(layer, devis_amd.ModulatedDeformableConv2d)
    argument_builders.unpatch_mask_head(seg, previous)
    assert seg.ModulatedDeformableConv2d is Theirs
    with pytest.raises(AttributeError):
        devis_amd.patch_mask_head(types.SimpleNamespace())


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _dcn_nodes(graph):
    return [n for n in graph.nodes if n.op == "call_function" and "deform_conv2d" in str(n.target)
            and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node_with_the_output_shape():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd.modules import ModulatedDeformableConv2d
    m = ModulatedDeformableConv2d(8, 4).to("meta")
    run = lambda m: make_fx(lambda p, x: torch.func.functional_call(m, p, (x,)), tracing_mode="fake")    # noqa: E731
    gm = run(m)(dict(m.named_parameters()), torch.empty(2, 8, 12, 20, device="meta"))
    nodes = _dcn_nodes(gm.graph)
    assert len(nodes) == 1 and tuple(nodes[0].meta["val"].shape) == (2, 4, 12, 20)
    assert nodes[0].meta["val"].dtype == torch.float32
    # stride 2, no padding, a 16-bit layer: the shape follows the convolution's formula
    m = ModulatedDeformableConv2d(8, 4, stride=2, padding=0).to("meta", torch.bfloat16)
    gm = run(m)(dict(m.named_parameters()), torch.empty(3, 8, 13, 20, device="meta", dtype=torch.bfloat16))
    val = _dcn_nodes(gm.graph)[0].meta["val"]
    assert tuple(val.shape) == (3, 4, 6, 9) and val.dtype == torch.bfloat16


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_for_static_and_dynamic_maps(dynamic):
    from devis_amd.modules import ModulatedDeformableConv2d
    m = ModulatedDeformableConv2d(8, 4, bias=True).to("meta")
    x = torch.empty(2, 8, 12, 20, device="meta")
    shapes = None
    if dynamic:
        shapes = ({2: torch.export.Dim("H", min=4, max=512), 3: torch.export.Dim("W", min=4, max=512)},)
    ep = torch.export.export(m, (x,), dynamic_shapes=shapes)
    nodes = _dcn_nodes(ep.graph)
    assert len(nodes) == 1
    val = nodes[0].meta["val"]
    assert val.shape[0] == 2 and val.shape[1] == 4
    if dynamic:
        assert str(val.shape[2]) == str(nodes[0].args[0].meta["val"].shape[2]) and not isinstance(val.shape[2], int)
        assert str(val.shape[3]) == str(nodes[0].args[0].meta["val"].shape[3])
    else:
        assert tuple(val.shape) == (2, 4, 12, 20)

"""CPU tests of the mask head's attention maps: the oracle against the reference fixtures, the C ABI of include/attmap.h
(exports, version, argument errors -- no compute calls), the host code (shape checks, errors, gradient masks), the module
and patch_attention_maps, and the fake-tensor paths.  The kernels themselves are tests/test_attmap_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch

import attmap_oracle
from conftest import ROOT, golden, golden_names

FIXTURES = golden_names("attmap_")
HEADS = 4


def load_fixture(name):
    d = {k: torch.from_numpy(v) for k, v in golden(name).items()}
    levels = len([k for k in d if k.startswith("k/")])
    state = {k[len("state/"):]: v for k, v in d.items() if k.startswith("state/")}
    masks = [d["mask/%d" % i] for i in range(levels)] if "mask/0" in d else None
    return d, levels, state, masks


# ---- oracle ----------------------------------------------------------------------------------------------------------

def test_fixtures_cover_the_cases():
    assert FIXTURES == ["attmap_masked", "attmap_nobias", "attmap_nomask"]
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 200 << 10
    d, levels, state, masks = load_fixture("attmap_nomask")
    assert levels == 3 and masks is None and d["q"].shape[:2] == (2, 5) and "q_linear_2.bias" in state
    d, levels, state, masks = load_fixture("attmap_nobias")
    assert masks is not None and sorted(state) == sorted("%s_linear%s.weight" % (a, s) for a in "qk" for s in ("", "_1", "_2"))


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference_outputs_and_gradients(name):
    d, levels, state, masks = load_fixture(name)
    q = d["q"].clone().requires_grad_(True)
    ks = [d["k/%d" % i].clone().requires_grad_(True) for i in range(levels)]
    params = {n: p.clone().requires_grad_(True) for n, p in state.items()}
    outs = attmap_oracle.module_forward(params, q, ks, masks, HEADS)
    for i, o in enumerate(outs):
        assert o.dtype == torch.float64 and float((o.detach() - d["out/%d" % i]).abs().max()) <= 1e-12
    leaves = [q] + ks + list(params.values())
    grads = torch.autograd.grad(outs, leaves, [d["grad_out/%d" % i] for i in range(levels)])
    want = [d["grad/q"]] + [d["grad/k/%d" % i] for i in range(levels)] + [d["grad/state/" + n] for n in params]
    for g, w in zip(grads, want):
        assert float((g - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max()))


def test_oracle_rows_sum_to_one_masked_pixels_are_zero_and_a_masked_row_is_nan():
    g = torch.Generator().manual_seed(3)
    q, k = torch.randn(2, 3, 8, generator=g, dtype=torch.float64), torch.randn(2, 8, 4, 5, generator=g, dtype=torch.float64)
    mask = torch.zeros(2, 4, 5, dtype=torch.bool)
    mask[0, :, 3:] = True
    out = attmap_oracle.attention_maps(q, k, mask, 2)
    assert out.shape == (2, 3, 2, 4, 5) and float((out.flatten(2).sum(-1) - 1).abs().max()) < 1e-14
    assert float(out[0, :, :, :, 3:].abs().max()) == 0.0
    mask[1] = True
    out = attmap_oracle.attention_maps(q, k, mask, 2)
    assert bool(out[1].isnan().all()) and not bool(out[0].isnan().any())


# ---- library ---------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_attmap_h_declares_and_versions_agree():
    from devis_amd import _attmap, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "attmap.h")).read()
    declared = set(re.findall(r"\b(attmap_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_attmap.EXPORTED_SYMBOLS) and len(declared) == 5
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _attmap.load()
    assert lib.attmap_version() == _attmap.ATTMAP_ABI_VERSION == int(re.search(r"#define ATTMAP_ABI_VERSION (\d+)", header).group(1))
    assert (_attmap.GRAD_Q, _attmap.GRAD_K) == tuple(
        int(re.search(r"#define ATTMAP_GRAD_%s (\d+)" % n, header).group(1)) for n in ("Q", "K"))
    codes = dict(re.findall(r"ATTMAP_(F32|F64|BF16|F16) = (\d)", header))
    assert codes == {"F32": "0", "F64": "1", "BF16": "2", "F16": "3"}
    assert os.path.join(build.include_dir(), "attmap.h") in build._headers()
    assert any(s.endswith("attmap.hip") for s in build.sources())


def _shape(**kw):
    from devis_amd import _attmap
    d = dict(B=2, Q=5, n=4, c=8, H=6, W=7)
    d.update(kw)
    return _attmap.Shape(**d)


def test_attmap_argument_errors_without_gpu():
    from devis_amd import _attmap
    lib = _attmap.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = ctypes.byref(_shape())
    err = lib.attmap_last_error
    assert lib.attmap_forward(0, 0, None, p, p, ok, 1.0, p, p, None) == -1 and b"null pointer" in err()
    assert lib.attmap_forward(0, 0, p, p, None, ok, 1.0, None, p, None) == -1 and b"null pointer" in err()
    assert lib.attmap_forward(0, 0, p, p, p, None, 1.0, p, p, None) == -1 and b"null pointer" in err()
    assert lib.attmap_forward(9, 9, p, p, p, ok, 1.0, p, p, None) == -1 and b"dtype" in err()
    # out_dtype: the inputs' type, or float32 beside 16-bit inputs -- nothing else
    for dt, odt in ((0, 2), (1, 0), (2, 3), (2, 1), (3, 2)):
        assert lib.attmap_forward(dt, odt, p, p, p, ok, 1.0, p, p, None) == -1 and b"out_dtype" in err(), (dt, odt)
    assert lib.attmap_forward(0, 0, p, p, p, ctypes.byref(_shape(n=0)), 1.0, p, p, None) == -1 and b"positive" in err()
    assert lib.attmap_forward(0, 0, p, p, p, ctypes.byref(_shape(Q=-1)), 1.0, p, p, None) == -1 and b"positive" in err()
    assert lib.attmap_forward(0, 0, p, p, p, ctypes.byref(_shape(c=513)), 1.0, p, p, None) == -1 and b"bound" in err()
    assert lib.attmap_forward(0, 0, p, p, p, ctypes.byref(_shape(H=65536, W=65536)), 1.0, p, p, None) == -1 and b"31 bits" in err()
    for empty in (_shape(Q=0), _shape(B=0)):        # no-op, nothing launched
        assert lib.attmap_forward(2, 0, None, None, None, ctypes.byref(empty), 1.0, None, None, None) == 0
        assert lib.attmap_backward(3, 2, 0, None, None, ctypes.byref(empty), 1.0, None, None, None) == 0
    assert lib.attmap_backward(3, 0, 0, p, None, ok, 1.0, p, p, None) == -1 and b"null pointer" in err()
    assert lib.attmap_backward(4, 0, 0, p, p, ok, 1.0, p, p, None) == -1 and b"grads" in err()
    assert lib.attmap_backward(1, 0, 2, p, p, ok, 1.0, p, p, None) == -1 and b"out_dtype" in err()
    assert lib.attmap_backward(0, 0, 0, None, None, ok, 1.0, None, None, None) == 0     # nothing asked for
    # two arithmetic values per (row, head, tile): 2*5 rows, 4 heads, one tile, rounded up to 256 bytes
    assert lib.attmap_workspace_bytes(0, ok) == 2 * 5 * 4 * 1 * 2 * 4 + 192
    assert lib.attmap_workspace_bytes(1, ok) == 2 * 5 * 4 * 1 * 2 * 8 + 128
    assert lib.attmap_workspace_bytes(2, ctypes.byref(_shape(H=100, W=167))) == 2 * 5 * 4 * 17 * 2 * 4 + 192
    assert lib.attmap_workspace_bytes(7, ok) == -1 and lib.attmap_workspace_bytes(0, None) == -1
    with pytest.raises(RuntimeError, match="positive"):
        _attmap.workspace_bytes(0, _shape(W=0))


def test_each_operator_keeps_an_error_message_of_its_own():
    """The four mask-path operators share the code of their error state, not the state: a failure of one leaves the
    others' <operator>_last_error() alone.  Run in a fresh thread, whose messages all start empty."""
    import threading
    from devis_amd import _attmap, _maskloss, _mdcn, _mhstage
    lib = _attmap.load()
    for binding in (_mdcn, _mhstage, _maskloss):
        assert binding.load() is lib
    last = {name: getattr(lib, name + "_last_error") for name in ("mdcn", "attmap", "mhstage", "maskloss")}
    seen = []

    def messages():
        return {name: f().decode() for name, f in last.items()}

    def run():
        seen.append(messages())
        try:
            _attmap.workspace_bytes(0, _shape(W=0))
        except RuntimeError as e:
            seen.append((str(e), messages()))
        assert lib.attmap_workspace_bytes(0, ctypes.byref(_shape())) > 0       # a good call clears the operator's message
        seen.append(messages())
        bad = _mdcn.Shape(N=1, C=8, H=6, W=7, Ho=6, Wo=7, Kh=3, Kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1,
                          dil_w=1, G=3)
        try:
            _mdcn.workspace_bytes(0, bad, 1)
        except RuntimeError as e:
            seen.append((str(e), messages()))

    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert len(seen) == 4, seen
    empty = dict.fromkeys(last, "")
    assert seen[0] == empty and seen[2] == empty
    text, after = seen[1]
    assert "positive" in after["attmap"] and text.endswith(after["attmap"]) and "attmap_workspace_bytes failed" in text
    assert after == dict(empty, attmap=after["attmap"])
    text, after = seen[3]
    assert "offset groups" in after["mdcn"] and text.endswith(after["mdcn"]) and "mdcn_workspace_bytes failed" in text
    assert after == dict(empty, mdcn=after["mdcn"])


# ---- host ------------------------------------------------------------------------------------------------------------

def test_operator_raises_on_cpu_tensors_and_on_bad_shapes_before_any_launch():
    import devis_amd
    from devis_amd.functions import attention_maps as A
    q, k = torch.zeros(2, 5, 32), torch.zeros(2, 32, 6, 7)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        devis_amd.attention_maps(q, k, num_heads=4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        A._backward(torch.zeros(2, 5, 4, 6, 7), q, k, torch.zeros(2, 5, 4, 6, 7), 4, 1.0, A.NEED_ALL)
    assert devis_amd.attention_maps is devis_amd.ops.attention_maps

    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="meta")      # noqa: E731
    q, k = meta(2, 5, 32), meta(2, 32, 6, 7)
    assert A.check_shapes(q, k, None, 4) == (2, 5, 4, 8, 6, 7, torch.float32)
    assert A.check_shapes(q, k, meta(2, 6, 7, dtype=torch.bool), 8)[:4] == (2, 5, 8, 4)
    h = torch.bfloat16
    assert A.check_shapes(meta(2, 5, 32, dtype=h), meta(2, 32, 6, 7, dtype=h), None, 4, torch.float32)[-1] == torch.float32
    assert A.check_shapes(meta(2, 5, 32, dtype=h), meta(2, 32, 6, 7, dtype=h), None, 4)[-1] == h
    with pytest.raises(RuntimeError, match="must be"):
        A.check_shapes(meta(5, 32), k, None, 4)
    with pytest.raises(RuntimeError, match="multiple of the 5 heads"):
        A.check_shapes(q, k, None, 5)
    with pytest.raises(RuntimeError, match="k must be"):
        A.check_shapes(q, meta(2, 16, 6, 7), None, 4)
    with pytest.raises(RuntimeError, match="k must be"):
        A.check_shapes(q, meta(3, 32, 6, 7), None, 4)
    with pytest.raises(RuntimeError, match="q's dtype"):
        A.check_shapes(q, meta(2, 32, 6, 7, dtype=h), None, 4)
    with pytest.raises(RuntimeError, match="mask must be"):
        A.check_shapes(q, k, meta(2, 7, 6, dtype=torch.bool), 4)
    with pytest.raises(RuntimeError, match="bool"):
        A.check_shapes(q, k, meta(2, 6, 7), 4)
    with pytest.raises(RuntimeError, match="out_dtype"):
        A.check_shapes(q, k, None, 4, torch.bfloat16)
    with pytest.raises(RuntimeError, match="out_dtype"):
        A.check_shapes(meta(2, 5, 32, dtype=h), meta(2, 32, 6, 7, dtype=h), None, 4, torch.float16)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        A.check_shapes(meta(2, 5, 32, dtype=torch.int32), meta(2, 32, 6, 7, dtype=torch.int32), None, 4)
    assert A.default_scale(q, 4) == 8 ** -0.5


def test_needs_input_grad_maps_to_the_gradient_mask():
    from devis_amd import _attmap, ops
    from devis_amd.functions import attention_maps as A
    from devis_amd.functions._common import op_runner
    assert (A.grads_mask(True, False), A.grads_mask(False, True), A.grads_mask(True, True)) == (1, 2, 3)
    assert (A.NEED_Q, A.NEED_K, A.NEED_ALL) == (_attmap.GRAD_Q, _attmap.GRAD_K, 3)
    seen = []
    q, k, out = torch.zeros(2, 5, 32), torch.zeros(2, 32, 6, 7), torch.zeros(2, 5, 4, 6, 7)

    def fake_op_backward(grad_out, q, k, out, num_heads, scale, grads):
        seen.append(("op", grads, num_heads, scale))
        return (torch.zeros_like(q) if grads & 1 else torch.zeros(0), torch.zeros_like(k) if grads & 2 else torch.zeros(0))

    def fake_host_backward(grad_out, q, k, out, num_heads, scale, grads):
        seen.append(("host", grads, num_heads, scale))
        return (torch.zeros_like(q) if grads & 1 else None, torch.zeros_like(k) if grads & 2 else None)

    # the one formula, run the way the op's register_autograd runs it and the way the eager Function does
    assert A.AttentionMapsFunction.setup_context is A.setup_context is ops.attention_maps_op._setup_context_fn
    assert ops.attention_maps_op._backward_fn.func is A.backward
    for needs, want in (((True, True, False, False, False, False), 3), ((True, False, False, False, False, False), 1),
                        ((False, True, False, False, False, False), 2)):
        ctx = types.SimpleNamespace(saved_tensors=(q, k, out), needs_input_grad=needs, num_heads=4, scale=0.5)
        res = A.backward(op_runner(fake_op_backward), ctx, out)
        assert seen[-1] == ("op", want, 4, 0.5) and len(res) == 6 and res[2:] == (None,) * 4
        assert (res[0] is not None, res[1] is not None) == needs[:2]
        res = A.backward(fake_host_backward, ctx, out)
        assert seen[-1] == ("host", want, 4, 0.5) and len(res) == 6 and res[2:] == (None,) * 4
        assert (res[0] is not None, res[1] is not None) == needs[:2]


# ---- module and patching ---------------------------------------------------------------------------------------------

def test_module_state_dict_initialisation_and_reference_checkpoint():
    from devis_amd.modules import MultiScaleMHAttentionMap
    m = MultiScaleMHAttentionMap(8, 32, HEADS, 3, dropout=0)
    keys = ["%s_linear%s.%s" % (a, s, w) for s in ("", "_1", "_2") for a in "qk" for w in ("weight", "bias")]
    assert list(m.state_dict()) == keys
    assert m.normalize_fact == 8 ** -0.5 and isinstance(m.dropout, torch.nn.Dropout)
    bound = (6.0 / (8 + 32)) ** 0.5         # xavier_uniform_
    for name, p in m.named_parameters():
        assert p.shape == ((32, 8) if name.endswith("weight") else (32,))
        if name.endswith("bias"):
            assert float(p.detach().abs().max()) == 0.0
        else:
            assert 0.5 * bound < float(p.detach().abs().max()) <= bound
    assert list(MultiScaleMHAttentionMap(8, 32, HEADS, 2, bias=False).state_dict()) == [
        "q_linear.weight", "k_linear.weight", "q_linear_1.weight", "k_linear_1.weight"]
    # the reference's checkpoints load strictly, and ours load into a module with the reference's layout
    for name, bias in (("attmap_masked", True), ("attmap_nobias", False)):
        _, levels, state, _ = load_fixture(name)
        m = MultiScaleMHAttentionMap(8, 32, HEADS, levels, bias=bias).double()
        m.load_state_dict(state, strict=True)
        assert torch.equal(m.k_linear_2.weight, state["k_linear_2.weight"])
        theirs = torch.nn.Module()
        for key in state:
            layer = key.split(".")[0]
            if not hasattr(theirs, layer):
                setattr(theirs, layer, torch.nn.Linear(8, 32, bias=bias).double())
        theirs.load_state_dict(m.state_dict(), strict=True)
    with pytest.raises(AssertionError):
        m.forward(torch.zeros(2, 5, 8), [torch.zeros(2, 8, 3, 4)] * 2)
    with pytest.raises(AssertionError):
        m.forward(torch.zeros(2, 5, 8), [torch.zeros(2, 8, 3, 4)] * 3, [torch.zeros(2, 3, 4, dtype=torch.bool)])


def test_patch_attention_maps_replaces_the_class_in_a_stand_in_module_and_leaves_the_convolution_alone():
    import devis_amd
    from devis_amd import argument_builders

    class Theirs(torch.nn.Module):
        pass

    class TheirConv(torch.nn.Module):
        pass

    seg = types.SimpleNamespace(MultiScaleMHAttentionMap=Theirs, ModulatedDeformableConv2d=TheirConv)
    previous = devis_amd.patch_attention_maps(seg)
    assert previous is Theirs and seg.MultiScaleMHAttentionMap is devis_amd.modules.MultiScaleMHAttentionMap
    assert seg.ModulatedDeformableConv2d is TheirConv
    layer = seg.MultiScaleMHAttentionMap(16, 16, 8, 3, dropout=0)
    assert isinstance(layer, devis_amd.MultiScaleMHAttentionMap)
    devis_amd.unpatch_attention_maps(seg, previous)
    assert seg.MultiScaleMHAttentionMap is Theirs
    # patch_mask_head stays what it was: the convolution only
    previous = devis_amd.patch_mask_head(seg)
    assert seg.MultiScaleMHAttentionMap is Theirs and seg.ModulatedDeformableConv2d is devis_amd.ModulatedDeformableConv2d
    argument_builders.unpatch_mask_head(seg, previous)
    with pytest.raises(AttributeError):
        devis_amd.patch_attention_maps(types.SimpleNamespace())


# ---- fake-tensor paths -----------------------------------------------------------------------------------------------

def _nodes(graph):
    return [n for n in graph.nodes if n.op == "call_function" and "attention_maps" in str(n.target)
            and "backward" not in str(n.target)]


def test_make_fx_with_fake_tensors_gives_one_op_node_with_the_output_shape():
    from torch.fx.experimental.proxy_tensor import make_fx
    from devis_amd import ops
    fn = lambda q, k, m: ops.attention_maps_op(q, k, m, 4, 0.25)      # noqa: E731
    gm = make_fx(fn, tracing_mode="fake")(torch.empty(2, 5, 32, device="meta"), torch.empty(2, 32, 12, 20, device="meta"),
                                          torch.empty(2, 12, 20, dtype=torch.bool, device="meta"))
    nodes = _nodes(gm.graph)
    assert len(nodes) == 1 and tuple(nodes[0].meta["val"].shape) == (2, 5, 4, 12, 20)
    assert nodes[0].meta["val"].dtype == torch.float32
    fn = lambda q, k: ops.attention_maps_op(q, k, None, 8, 0.5, torch.float32)      # noqa: E731
    gm = make_fx(fn, tracing_mode="fake")(torch.empty(3, 7, 32, device="meta", dtype=torch.bfloat16),
                                          torch.empty(3, 32, 13, 21, device="meta", dtype=torch.bfloat16))
    val = _nodes(gm.graph)[0].meta["val"]
    assert tuple(val.shape) == (3, 7, 8, 13, 21) and val.dtype == torch.float32


@pytest.mark.parametrize("dynamic", [False, True])
def test_export_gives_one_op_node_per_level_for_static_and_dynamic_maps(dynamic):
    from devis_amd.modules import MultiScaleMHAttentionMap
    m = MultiScaleMHAttentionMap(16, 32, HEADS, 1).to("meta")

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = m

        def forward(self, q, k, mask):
            return self.m(q, [k], [mask])[0]

    q, k = torch.empty(2, 5, 16, device="meta"), torch.empty(2, 16, 12, 20, device="meta")
    mask = torch.empty(2, 12, 20, dtype=torch.bool, device="meta")
    shapes = None
    if dynamic:
        Q, H, W = torch.export.Dim("Q", min=2, max=512), torch.export.Dim("H", min=4, max=512), torch.export.Dim("W", min=4, max=512)
        shapes = ({1: Q}, {2: H, 3: W}, {1: H, 2: W})
    ep = torch.export.export(Wrap(), (q, k, mask), dynamic_shapes=shapes)
    nodes = _nodes(ep.graph)
    assert len(nodes) == 1
    val = nodes[0].meta["val"]
    assert val.shape[0] == 2 and val.shape[2] == HEADS and len(val.shape) == 5
    if dynamic:
        assert not any(isinstance(val.shape[d], int) for d in (1, 3, 4))
    else:
        assert tuple(val.shape) == (2, 5, HEADS, 12, 20)

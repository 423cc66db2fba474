"""torch.compile / torch.export of the operator and the modules, on the CPU (no GPU): the custom ops of devis_amd/ops.py
are checked with torch.library.opcheck, and compiled calls are compared with eager calls.  Where kernels must run, the
oracle-backed double of tests/fake_native.py stands in for the library (plus a torch restatement of the fused pre-op pass,
below); tracing and export need no kernels at all."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
from torch._dynamo.testing import CompileCounterWithBackend
from torch.utils._python_dispatch import TorchDispatchMode

import fake_native
import module_cases
from conftest import ROOT, golden


@pytest.fixture(autouse=True)
def _fresh_dynamo():
    torch._dynamo.reset()
    torch._dynamo.utils.counters.clear()
    yield
    torch._dynamo.reset()


def _op_inputs(name, grad=True):
    g = golden(name)
    v, l, a = (torch.from_numpy(g[k]).double().requires_grad_(grad)
               for k in ("value", "sampling_locations", "attention_weights"))
    return g, v, torch.from_numpy(g["spatial_shapes"]), torch.from_numpy(g["level_start_index"]), l, a


def _temporal_op_inputs(monkeypatch, name):
    """The arguments the fused temporal call of module case `name` hands to the library (captured from an eager run on
    the double), in fp64."""
    fake_native.install(monkeypatch)
    from devis_amd import _native
    seen = {}
    inner = _native.temporal_forward

    def capture(value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t, clips, out):
        seen["args"] = [t.detach().clone() for t in (value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t)] + [clips]
        inner(value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t, clips, out)

    monkeypatch.setattr(_native, "temporal_forward", capture)
    module_cases.run(name, "cpu", torch.float64, fused=True)
    monkeypatch.setattr(_native, "temporal_forward", inner)
    args = seen["args"]
    args[0] = args[0].contiguous()
    return args


def _install_prep_double(monkeypatch):
    """msda_prep_forward / msda_prep_backward restated in torch ops (the arithmetic of ref ms_deform_attn.py:112-121 and
    :252-258), writing into the buffers the host code hands over -- the contract of include/msda.h, for CPU tensors."""
    from devis_amd import _native

    def levels(shapes, LL, L):
        wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(torch.float64)
        return wh.repeat(LL // L, 1)                                   # slot-major, level-minor

    def loc_of(off, ref, shapes, L, P):
        off, ref = off.double(), ref.double()
        if ref.shape[-1] == 2:
            return ref[:, None, :, None, :] + off / levels(shapes, off.shape[2], L)[None, None, :, None, :]
        return ref[:, None, :, None, :2] + off / P * ref[:, None, :, None, 2:] * 0.5

    def prep_forward(off_c, off_t, logit_c, logit_t, ref_c, ref_t, shapes, R, M, L, W, Pc, Pt,
                     loc_c, loc_t, aw_c, aw_t, ld=0):
        oc = off_c.reshape(R, M, L, Pc, 2)
        logits = [logit_c.reshape(R, M, L * Pc).double()]
        loc_c.copy_(loc_of(oc, ref_c, shapes, L, Pc))
        if W:
            loc_t.copy_(loc_of(off_t.reshape(R, M, W * L, Pt, 2), ref_t, shapes, L, Pt))
            logits.append(logit_t.reshape(R, M, W * L * Pt).double())
        a = torch.softmax(torch.cat(logits, -1), -1)
        aw_c.copy_(a[..., :L * Pc].reshape(aw_c.shape))
        if W:
            aw_t.copy_(a[..., L * Pc:].reshape(aw_t.shape))

    def goff_of(gloc, ref, shapes, L, P):
        gloc, ref = gloc.double(), ref.double()
        if ref.shape[-1] == 2:
            return gloc / levels(shapes, gloc.shape[2], L)[None, None, :, None, :]
        return gloc / P * ref[:, None, :, None, 2:] * 0.5

    def prep_backward(gloc_c, gloc_t, gaw_c, gaw_t, aw_c, aw_t, ref_c, ref_t, shapes, R, M, L, W, Pc, Pt,
                      goff_c, goff_t, glogit_c, glogit_t, ld=0):
        goff_c.copy_(goff_of(gloc_c, ref_c, shapes, L, Pc).reshape(goff_c.shape))
        a, g = [aw_c.reshape(R, M, -1).double()], [gaw_c.reshape(R, M, -1).double()]
        if W:
            goff_t.copy_(goff_of(gloc_t, ref_t, shapes, L, Pt).reshape(goff_t.shape))
            a.append(aw_t.reshape(R, M, -1).double())
            g.append(gaw_t.reshape(R, M, -1).double())
        a, g = torch.cat(a, -1), torch.cat(g, -1)
        gl = a * (g - (a * g).sum(-1, keepdim=True))
        glogit_c.copy_(gl[..., :L * Pc].reshape(glogit_c.shape))
        if W:
            glogit_t.copy_(gl[..., L * Pc:].reshape(glogit_t.shape))

    monkeypatch.setattr(_native, "prep_forward", prep_forward)
    monkeypatch.setattr(_native, "prep_backward", prep_backward)
    from devis_amd.functions import ms_deform_attn_func as F
    real = F._check_prep_inputs
    monkeypatch.setattr(F, "_check_prep_inputs", lambda y, refs, shapes, sdt=None: [
        None if r is None else r.to(sdt or y.dtype).contiguous() for _, r in refs] if not y.is_cuda else real(y, refs, shapes, sdt))


# ---- 1. opcheck -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["op_batched_im2col", "op_many_levels"])
def test_opcheck_ms_deform_attn_ops(monkeypatch, name):
    fake_native.install(monkeypatch)
    from devis_amd import ops
    g, v, ss, lsi, l, a = _op_inputs(name)
    torch.library.opcheck(ops.ms_deform_attn_forward, (v, ss, lsi, l, a, 2 if v.shape[0] % 2 == 0 else 1))
    mask = torch.zeros(v.shape[:2], dtype=torch.bool)
    mask[:, ::3] = True
    torch.library.opcheck(ops.ms_deform_attn_forward, (v, ss, lsi, l, a, 64, mask, True))
    go = torch.from_numpy(g["grad_output"])
    for m in (None, mask):
        torch.library.opcheck(ops.ms_deform_attn_backward, (v.detach(), ss, lsi, l.detach(), a.detach(), go, 64, m))
    gv, gl, ga = ops.ms_deform_attn_backward(v.detach(), ss, lsi, l.detach(), a.detach(), go, 64)
    np.testing.assert_allclose(gv.numpy(), g["grad_value"], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("name", ["mod_temporal_enc", "mod_temporal_dec_ref2"])
def test_opcheck_temporal_ops(monkeypatch, name):
    from devis_amd import ops
    value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t, clips = _temporal_op_inputs(monkeypatch, name)
    leaves = [t.requires_grad_(True) for t in (value, loc_c, aw_c, loc_t, aw_t)]
    torch.library.opcheck(ops.temporal_forward, (value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t, clips))
    go = torch.randn(value.shape[0], loc_c.shape[1], value.shape[2] * value.shape[3], dtype=torch.float64)
    det = [t.detach() for t in leaves]
    torch.library.opcheck(ops.temporal_backward, (det[0], shapes, lsi, ftab, det[1], det[2], det[3], det[4], go, clips))


def _prep_case(name, W, d):
    """Offsets / logits / reference points shaped like module case `name` (M heads, L levels, 3 current and 2 temporal
    points), drawn from the fixture's own query."""
    g = golden(name)
    M, L, Pc, Pt = module_cases.M, module_cases.L, 3, 2
    q = torch.from_numpy(g["in/query"]).double().reshape(-1, module_cases.C)
    R = q.shape[0]
    gen = torch.Generator().manual_seed(5)
    proj = lambda n: q @ torch.randn(module_cases.C, n, generator=gen, dtype=torch.float64) * 0.3
    shapes = torch.from_numpy(g["in/spatial_shapes/0"] if "in/spatial_shapes/0" in g else g["in/spatial_shapes"])
    ref_c = torch.rand(R, L, d, generator=gen, dtype=torch.float64) * 0.8 + 0.1
    ref_t = torch.rand(R, W * L, d, generator=gen, dtype=torch.float64) * 0.8 + 0.1 if W else None
    return dict(y=proj(M * L * Pc * 2 + M * W * L * Pt * 2 + M * L * Pc + M * W * L * Pt), ref_c=ref_c, ref_t=ref_t,
                shapes=shapes, dims=(M, L, W, Pc, Pt))


@pytest.mark.parametrize("W,d", [(0, 2), (2, 2), (2, 4)])
def test_opcheck_prep_ops(monkeypatch, W, d):
    _install_prep_double(monkeypatch)
    from devis_amd import ops
    from devis_amd.functions import MSDeformPrepFusedFunction
    c = _prep_case("mod_temporal_dec_ref2", W, d)
    M, L, W, Pc, Pt = c["dims"]
    y = c["y"].requires_grad_(True)
    ref_c = c["ref_c"].requires_grad_(True)
    ref_t = c["ref_t"].requires_grad_(True) if W else None
    torch.library.opcheck(ops.prep_fused_forward, (y, ref_c, ref_t, c["shapes"], M, L, W, Pc, Pt, False))
    cols = MSDeformPrepFusedFunction._cols(M, L, W, Pc, Pt)
    R = y.shape[0]
    off_c = y[:, cols[0][0]:cols[0][1]].detach().reshape(R, M, L, Pc, 2).requires_grad_(True)
    logit_c = y[:, cols[2][0]:cols[2][1]].detach().reshape(R, M, L * Pc).requires_grad_(True)
    off_t = y[:, cols[1][0]:cols[1][1]].detach().reshape(R, M, W * L, Pt, 2).requires_grad_(True) if W else None
    logit_t = y[:, cols[3][0]:cols[3][1]].detach().reshape(R, M, W * L * Pt).requires_grad_(True) if W else None
    torch.library.opcheck(ops.prep_forward, (off_c, off_t, logit_c, logit_t, ref_c, ref_t, c["shapes"], False))
    loc_c, loc_t, aw_c, aw_t = (t.detach() for t in ops.prep_forward(off_c, off_t, logit_c, logit_t, ref_c, ref_t,
                                                                       c["shapes"], False))
    grads = [torch.randn_like(t) for t in (loc_c, loc_t, aw_c, aw_t)]
    det = lambda t: None if t is None else t.detach()
    torch.library.opcheck(ops.prep_backward, (*grads, aw_c, aw_t if W else None, det(off_c), det(off_t), det(ref_c),
                                              det(ref_t), c["shapes"], False, True, bool(W)))
    torch.library.opcheck(ops.prep_fused_backward, (*grads, aw_c, aw_t if W else None, y.detach(), det(ref_c), det(ref_t),
                                                    c["shapes"], M, L, W, Pc, Pt, False, True, bool(W)))
    # the op and the Function agree with the torch ops of the modules' unfused path
    got = MSDeformPrepFusedFunction.apply(y, ref_c, ref_t, c["shapes"], M, L, W, Pc, Pt)
    for a, b in zip(got, ops.prep_fused_forward(y, ref_c, ref_t, c["shapes"], M, L, W, Pc, Pt)):
        if a is not None:
            assert torch.equal(a, b)


@pytest.mark.parametrize("W,d", [(0, 2), (2, 4)])
def test_prep_functions_compile_fullgraph_and_match_eager(monkeypatch, W, d):
    """The compile branches of MSDeformPrepFusedFunction / MSDeformPrepFunction (the modules take them on the GPU)."""
    _install_prep_double(monkeypatch)
    from devis_amd.functions import MSDeformPrepFunction, MSDeformPrepFusedFunction
    c = _prep_case("mod_temporal_dec_ref4", W, d)
    M, L, W, Pc, Pt = c["dims"]
    cols = MSDeformPrepFusedFunction._cols(M, L, W, Pc, Pt)
    R = c["y"].shape[0]

    def fused(y, ref_c, ref_t):
        return MSDeformPrepFusedFunction.apply(y, ref_c, ref_t, c["shapes"], M, L, W, Pc, Pt)

    def unfused(y, ref_c, ref_t):
        part = lambda i, shape: y[:, cols[i][0]:cols[i][1]].reshape(shape)
        return MSDeformPrepFunction.apply(part(0, (R, M, L, Pc, 2)), part(1, (R, M, W * L, Pt, 2)) if W else None,
                                          part(2, (R, M, L * Pc)), part(3, (R, M, W * L * Pt)) if W else None,
                                          ref_c, ref_t, c["shapes"])

    for fn in (fused, unfused):
        res = []
        for f in (fn, torch.compile(fn, fullgraph=True, backend="aot_eager")):
            leaves = [c["y"].clone().requires_grad_(True), c["ref_c"].clone().requires_grad_(True)] + \
                ([c["ref_t"].clone().requires_grad_(True)] if W else [])
            outs = [o for o in f(*leaves, *([] if W else [None])) if o is not None]
            loss = sum((o * torch.linspace(-1, 1, o.numel(), dtype=o.dtype).view(o.shape)).sum() for o in outs)
            res.append([o.detach() for o in outs] + list(torch.autograd.grad(loss, leaves)))
        assert len(res[0]) == len(res[1]) == (4 if W else 2) + len(leaves)
        for a, b in zip(*res):
            assert torch.equal(a, b)
    assert not torch._dynamo.utils.counters["graph_break"]


def test_opcheck_frame_table():
    from devis_amd import ops
    offs = [torch.tensor([1, 2]), torch.tensor([-1, 1]), torch.tensor([-2, -1])]
    torch.library.opcheck(ops.frame_table, (offs, 3, torch.device("cpu")))
    assert ops.frame_table(offs, 3, torch.device("cpu")).tolist() == [[1, 2], [0, 2], [0, 1]]


def test_every_op_keeps_its_recorded_schema():
    """The ops of the namespace and their schemas are an outward contract (saved graphs and exported programs name them):
    tests/golden/op_schemas.json is the list, recorded before the autograd formulas moved next to the host code."""
    import json
    from devis_amd import ops
    with open(os.path.join(ROOT, "tests", "golden", "op_schemas.json")) as f:
        want = json.load(f)
    prefix = ops.NAMESPACE + "::"
    names = sorted({n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(prefix)})
    got = [str(getattr(getattr(torch.ops, ops.NAMESPACE), n[len(prefix):]).default._schema).replace(prefix, "devis_amd::", 1)
           for n in names]
    assert len(want) == 34 and got == want


# ---- 2. the Function under torch.compile ----------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 64])
def test_function_compiles_fullgraph_and_matches_eager_bit_for_bit(monkeypatch, step):
    fake_native.install(monkeypatch)
    from devis_amd.functions import MSDeformAttnFunction

    def f(v, ss, lsi, l, a):
        return MSDeformAttnFunction.apply(v, ss, lsi, l, a, step)

    res = []
    for fn in (f, torch.compile(f, fullgraph=True, backend="aot_eager")):
        g, v, ss, lsi, l, a = _op_inputs("op_batched_im2col")
        out = fn(v, ss, lsi, l, a)
        res.append((out.detach(),) + torch.autograd.grad(out, (v, l, a), torch.from_numpy(g["grad_output"])))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    out, gv, gl, ga = res[1]
    np.testing.assert_allclose(out.numpy(), g["out"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gv.numpy(), g["grad_value"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(gl.numpy(), g["grad_sampling_loc"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ga.numpy(), g["grad_attn_weight"], rtol=1e-11, atol=1e-14)
    assert not torch._dynamo.utils.counters["graph_break"]


def test_temporal_function_compiles_fullgraph(monkeypatch):
    from devis_amd.functions import MSDeformAttnTemporalFunction
    args = _temporal_op_inputs(monkeypatch, "mod_temporal_dec_ref2")
    go = torch.randn(args[0].shape[0], args[4].shape[1], args[0].shape[2] * args[0].shape[3], dtype=torch.float64)
    f = MSDeformAttnTemporalFunction.apply
    res = []
    for fn in (f, torch.compile(f, fullgraph=True, backend="aot_eager")):
        a = [t.clone().requires_grad_(True) if i in (0, 4, 5, 6, 7) else t for i, t in enumerate(args)]
        out = fn(*a)
        res.append((out.detach(),) + torch.autograd.grad(out, [a[i] for i in (0, 4, 5, 6, 7)], go))
    for x, y in zip(*res):
        assert torch.equal(x, y)


# ---- 3. the modules under torch.compile -----------------------------------------------------------------------------

def _module_inputs(name, g):
    t = lambda key: module_cases._t(g, key, "cpu", torch.float64)
    query, src, ref = t("in/query").requires_grad_(True), t("in/input_flatten").requires_grad_(True), t("in/reference_points")
    if name.startswith("mod_plain"):
        return [query, ref, src, t("in/spatial_shapes"), t("in/level_start_index"), t("in/padding_mask")]
    n = len([k for k in g if k.startswith("in/temporal_offsets/")])
    return [query, ref, src, tuple(t("in/spatial_shapes/%d" % i) for i in range(2)),
            tuple(t("in/level_start_index/%d" % i) for i in range(2)), [t("in/temporal_offsets/%d" % i) for i in range(n)]]


def _run_module(mod, fn, args, w):
    args = [a.detach().clone().requires_grad_(a.requires_grad) if isinstance(a, torch.Tensor) else a for a in args]
    ret = fn(*args)
    params = [p for _, p in sorted(mod.named_parameters())]
    grads = torch.autograd.grad((ret[0] * w).sum(), [args[0], args[2]] + params)
    flat = [ret[0]] + [x for r in ret[1:] if r is not None for x in (r if isinstance(r, list) else [r])]
    return [x.detach() for x in flat] + list(grads)


MODULE_CASES = ["mod_plain_ref2", "mod_plain_ref4", "mod_temporal_enc", "mod_temporal_enc_window",
                "mod_temporal_dec_ref2", "mod_temporal_dec_ref4", "mod_temporal_dec_not_instance_aware",
                "mod_temporal_dec_ref4_not_instance_aware"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", MODULE_CASES)
def test_modules_compile_fullgraph_and_match_eager(monkeypatch, name, fused):
    if name.startswith("mod_plain") and not fused:
        pytest.skip("plain module has a single call pattern")
    fake_native.install(monkeypatch)
    mod, g = module_cases.build(name, "cpu", torch.float64)
    if hasattr(mod, "fused"):
        mod.fused = fused
    args, w = _module_inputs(name, g), module_cases._t(g, "loss_weight", "cpu", torch.float64)
    eager = _run_module(mod, mod, args, w)
    compiled = _run_module(mod, torch.compile(mod, fullgraph=True, backend="aot_eager"), args, w)
    assert len(eager) == len(compiled)
    for a, b in zip(eager, compiled):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    assert not torch._dynamo.utils.counters["graph_break"]


# ---- 4. dynamic pyramids --------------------------------------------------------------------------------------------

def _pyramid_args(shapes, seed, C=32, L=2, Lq=5):
    gen = torch.Generator().manual_seed(seed)
    ss = torch.tensor(shapes, dtype=torch.long)
    lsi = torch.cat((ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1]))
    S = int(ss.prod(1).sum())
    mask = torch.rand(1, S, generator=gen) < 0.2
    return [torch.randn(1, Lq, C, generator=gen, dtype=torch.float64), torch.rand(1, Lq, L, 2, generator=gen, dtype=torch.float64),
            torch.randn(1, S, C, generator=gen, dtype=torch.float64), ss, lsi, mask]


def test_dynamic_pyramids_compile_at_most_twice_without_graph_breaks(monkeypatch):
    fake_native.install(monkeypatch)
    from devis_amd.modules import MSDeformAttn
    torch.manual_seed(0)
    mod = MSDeformAttn(32, 2, 4, 3).double()
    cnt = CompileCounterWithBackend("aot_eager")
    cmod = torch.compile(mod, fullgraph=True, backend=cnt)
    for shapes, seed in (([(6, 4), (3, 2)], 1), ([(8, 5), (4, 3)], 2), ([(6, 4), (3, 2)], 3)):
        args = _pyramid_args(shapes, seed)
        args[0].requires_grad_(True)
        args[2].requires_grad_(True)
        w = torch.randn(1, 5, 32, dtype=torch.float64)
        eager, compiled = _run_module(mod, mod, args, w), _run_module(mod, cmod, args, w)
        for a, b in zip(eager, compiled):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    assert not torch._dynamo.utils.counters["graph_break"]
    assert cnt.frame_count <= 2
    with pytest.raises(AssertionError):                  # ref :96, now checked inside the op at run time
        bad = _pyramid_args([(6, 4), (3, 2)], 4)
        bad[3] = torch.tensor([[6, 4], [3, 3]])
        cmod(*bad)


# ---- 5. temporal offsets: new tensors every call, never a stale table -----------------------------------------------

def test_compiled_decoder_follows_new_offset_tensors_and_raises_on_bad_ones(monkeypatch):
    fake_native.install(monkeypatch)
    name = "mod_temporal_dec_ref2"
    mod, g = module_cases.build(name, "cpu", torch.float64)
    args, w = _module_inputs(name, g), module_cases._t(g, "loss_weight", "cpu", torch.float64)
    cmod = torch.compile(mod, fullgraph=True, backend="aot_eager")
    T = len(args[5])
    other = [torch.tensor([t for t in range(-f, T - f) if t != 0][::-1]) for f in range(T)]       # same shape, other frames
    for offs in ([o.clone() for o in args[5]], [o.clone() for o in args[5]], other):
        args[5] = offs
        eager = _run_module(mod, mod, args, w)
        compiled = _run_module(mod, cmod, args[:5] + [[o.clone() for o in offs]], w)      # new tensors again
        for a, b in zip(eager, compiled):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    args[5] = [torch.tensor([1, 7])] * T
    with pytest.raises(IndexError, match="outside the clip"):
        mod(*args)
    with pytest.raises(IndexError, match="outside the clip"):
        cmod(*args)


# ---- 6. torch.export ------------------------------------------------------------------------------------------------

def test_export_plain_module_without_kernels_then_run_it(monkeypatch):
    from devis_amd.modules import MSDeformAttn
    torch.manual_seed(0)
    mod = MSDeformAttn(32, 2, 4, 3).double().eval()
    args = tuple(_pyramid_args([(6, 4), (3, 2)], 1))
    ep = torch.export.export(mod, args)
    assert "devis_amd.ms_deform_attn_forward" in str(ep.graph)
    fake_native.install(monkeypatch)
    got, want = ep.module()(*args), mod(*args)
    assert got[1] is None and torch.allclose(got[0], want[0], rtol=1e-12, atol=1e-14)


# ---- 7. eager dispatches no custom op -------------------------------------------------------------------------------

class _Record(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.add(str(func))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("name", ["mod_plain_ref2", "mod_temporal_enc", "mod_temporal_dec_ref2"])
def test_eager_modules_dispatch_no_custom_op(monkeypatch, name):
    fake_native.install(monkeypatch)
    with _Record() as rec:
        module_cases.run(name, "cpu", torch.float64, fused=True)
    assert rec.ops and not [op for op in rec.ops if "devis_amd" in op]


# ---- 8. error contract under compile --------------------------------------------------------------------------------

def _error(fn, *args):
    with pytest.raises(RuntimeError) as e:
        fn(*args)
    return str(e.value)


def test_compiled_calls_raise_the_eager_errors(monkeypatch):
    from devis_amd.functions import MSDeformAttnFunction
    g, v, ss, lsi, l, a = _op_inputs("op_batched_im2col", grad=False)
    f = lambda v, l, a, step: MSDeformAttnFunction.apply(v, ss, lsi, l, a, step)
    cf = torch.compile(f, fullgraph=True, backend="aot_eager")
    msg = _error(f, v, l, a, 2)
    assert "Not implemented on the CPU" in msg and msg in _error(cf, v, l, a, 2)
    fake_native.install(monkeypatch)
    torch._dynamo.reset()
    msg = _error(f, v, l, a, 4)
    assert "must divide" in msg and msg in _error(cf, v, l, a, 4)
    l_nc = l.transpose(1, 2).contiguous().transpose(1, 2)
    msg = _error(f, v, l_nc, a, 2)
    assert "sampling_loc tensor has to be contiguous" in msg and msg in _error(cf, v, l_nc, a, 2)


def test_second_derivative_raises_as_in_eager(monkeypatch):
    fake_native.install(monkeypatch)
    from devis_amd import ops
    g, v, ss, lsi, l, a = _op_inputs("op_batched_im2col")
    out = ops.ms_deform_attn_forward(v, ss, lsi, l, a, 64)
    gv, = torch.autograd.grad(out.sum(), (v,), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gv.sum(), (l,))


# ---- 9. path B: integration/MultiScaleDeformableAttention.py --------------------------------------------------------

def test_path_b_reference_function_exports_through_the_stub_op(tmp_path):
    try:
        from devis_amd import build
        build.ensure()
    except Exception as e:  # noqa: BLE001
        pytest.skip("the HIP library cannot be built here: %s" % e)
    from test_dropin import _reference_shaped_function
    sys.path.insert(0, os.path.join(ROOT, "integration"))
    try:
        sys.modules.pop("MultiScaleDeformableAttention", None)
        msda = importlib.import_module("MultiScaleDeformableAttention")
        fn = _reference_shaped_function(msda)

        class Call(torch.nn.Module):
            def forward(self, v, ss, lsi, l, a):
                return fn.apply(v, ss, lsi, l, a, 2)

        g, v, ss, lsi, l, a = _op_inputs("op_batched_im2col", grad=False)
        ep = torch.export.export(Call(), (v, ss, lsi, l, a))
        assert "MultiScaleDeformableAttention" in str(ep.graph) and "ms_deform_attn_forward" in str(ep.graph)
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):        # ms_deform_attn.h:38, at run time
            ep.module()(v, ss, lsi, l, a)
    finally:
        sys.path.remove(os.path.join(ROOT, "integration"))
        sys.modules.pop("MultiScaleDeformableAttention", None)

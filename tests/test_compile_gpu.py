"""torch.compile (Inductor, fullgraph) and torch.export of the operator, the modules and path B on the GPU: the custom ops of
devis_amd/ops.py run the same HIP kernels as eager.  Op-level results are bit-identical to eager (grad_value: as repeatable
as eager's own float atomics); module-level results
(where Inductor compiles the Linears, the softmax and the arithmetic around the operator) are within the module
tolerances.  About seven Inductor compilations in all."""
import importlib
import os
import sys

import pytest
import torch
from torch._dynamo.testing import CompileCounterWithBackend

from conftest import ROOT
from helpers import PYR_A, make_inputs, make_temporal_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fresh_dynamo():
    torch._dynamo.reset()
    torch._dynamo.utils.counters.clear()
    yield
    torch._dynamo.reset()


def _eager_and_compiled(fn, args, grad_idx, grad_out):
    """[(out, *grads)] of fn eager, eager again and compiled (inductor, fullgraph), plus the route of each forward."""
    from devis_amd import _native
    res, routes = [], []
    for f in (fn, fn, torch.compile(fn, fullgraph=True, backend="inductor")):
        a = [x.clone().requires_grad_(True) if i in grad_idx else x for i, x in enumerate(args)]
        out = f(*a)
        torch.cuda.synchronize()
        routes.append(_native.last_route())
        res.append([out.detach()] + list(torch.autograd.grad(out, [a[i] for i in grad_idx], grad_out)))
    return res, routes


def _assert_same_as_eager(res):
    """Compiled == eager bit for bit wherever two eager calls agree bit for bit.  grad_value is summed with float atomics
    on several backward routes (the order of the additions varies from call to call); where the two eager calls differ,
    the compiled one must differ from eager no more than they do (x2), and never by more than 1e-5 / 1e-2 (bf16) of scale."""
    eager, again, compiled = res
    for k, (a, b, c) in enumerate(zip(eager, again, compiled)):
        assert a.dtype == c.dtype and a.shape == c.shape, k
        if torch.equal(a, b):
            assert torch.equal(a, c), k
        else:
            spread = float((a.float() - b.float()).abs().max())
            err = float((a.float() - c.float()).abs().max())
            bound = (1e-2 if a.dtype == torch.bfloat16 else 1e-5) * max(1.0, float(a.float().abs().max()))
            assert k == 1 and err <= max(2 * spread, 1e-30) and err <= bound, (k, err, spread)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_temporal_function_under_inductor_is_bit_identical(dtype):
    """A cfg3-shaped decoder call: 2 clips of T = 6 frames, 300 queries, pyramid A, D = 32."""
    from devis_amd.functions import MSDeformAttnTemporalFunction
    d = make_temporal_inputs(11, T=6, W=5, M=8, D=32, Lq=300, shapes=PYR_A, Pc=4, Pt=4)
    clips = 2
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    for k in ("value", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out"):
        t[k] = torch.cat([t[k], t[k].flip(0)]).to(dtype if k in ("value", "grad_out") else torch.float32)
    args = [t[k] for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t")] + [clips]
    res, routes = _eager_and_compiled(MSDeformAttnTemporalFunction.apply, args, (0, 4, 5, 6, 7), t["grad_out"])
    assert routes[0] == routes[2] and "msda" in routes[0], routes
    _assert_same_as_eager(res)
    assert not torch._dynamo.utils.counters["graph_break"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_function_under_inductor_is_bit_identical_generic_d(dtype):
    from devis_amd.functions import MSDeformAttnFunction
    d = make_inputs(12, N=2, M=8, D=64, Lq=300, shapes=PYR_A, P=4)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    args = [t["value"].to(dtype), t["shapes"], t["lsi"], t["loc"], t["aw"]]
    fn = lambda v, ss, lsi, l, a: MSDeformAttnFunction.apply(v, ss, lsi, l, a, 64)
    res, routes = _eager_and_compiled(fn, args, (0, 3, 4), t["grad_out"].to(dtype))
    assert routes[0] == routes[2] and "msda" in routes[0], routes
    _assert_same_as_eager(res)


def _layers():
    """MSDeformAttn (2 images, padding mask), TemporalMSDeformAttnEncoder (small pyramid) and TemporalMSDeformAttnDecoder
    (cfg3-shaped) with random parameters, fp32."""
    from devis_amd.modules import MSDeformAttn, TemporalMSDeformAttnDecoder, TemporalMSDeformAttnEncoder
    torch.manual_seed(0)
    T, C = 6, 256
    layers = [MSDeformAttn(C, 4, 8, 4), TemporalMSDeformAttnEncoder(3, C, 4, 2, 8, 4, 4),
              TemporalMSDeformAttnDecoder(T, C, 4, T - 1, 8, 4, 4)]
    with torch.no_grad():
        for m in layers:
            for n, p in m.named_parameters():
                p.normal_(0, 0.02 if "sampling_offsets.weight" in n else 0.05)
    return [m.to(DEV) for m in layers]


def _pyramid(shapes, frames):
    ss = torch.tensor(shapes, dtype=torch.long, device=DEV)
    lsi = torch.cat((ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1]))
    t_ss = ss.repeat(frames - 1, 1)
    t_lsi = torch.cat((t_ss.new_zeros(1), t_ss.prod(1).cumsum(0)[:-1]))
    return ss, lsi, t_ss, t_lsi, int(ss.prod(1).sum())


def _layer_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen).to(DEV).requires_grad_(True)
    rnd = lambda *s: (torch.rand(*s, generator=gen) * 0.8 + 0.1).to(DEV)
    ss, lsi, _, _, S = _pyramid(PYR_A, 2)
    plain = [mk(2, 300, 256), rnd(2, 300, 4, 2), mk(2, S, 256), ss, lsi, (torch.rand(2, S, generator=gen) < 0.05).to(DEV)]
    small = [(16, 24), (8, 12), (4, 6), (2, 3)]
    ess, elsi, ets, etl, eS = _pyramid(small, 3)
    centres = rnd(1, eS, 1, 2).expand(3, eS, 4, 2).contiguous()
    enc = [mk(3, eS, 256), centres, mk(3, eS, 256), (ess, ets), (elsi, etl),
           [torch.tensor([t for t in range(-f, 3 - f) if t != 0], device=DEV) for f in range(3)]]
    dss, dlsi, dts, dtl, dS = _pyramid(PYR_A, 6)
    dec = [mk(1, 6 * 300, 256), rnd(1, 6 * 300, 4, 2), mk(6, dS, 256), (dss, dts), (dlsi, dtl),
           [torch.tensor([t for t in range(-f, 6 - f) if t != 0], device=DEV) for f in range(6)]]     # new tensors each call
    return [plain, enc, dec]


def _step(layers, inputs):
    return [m(*a)[0] for m, a in zip(layers, inputs)]


def _grads(layers, inputs, outs, weights):
    loss = sum((o.float() * w).sum() for o, w in zip(outs, weights))
    leaves = [a[i] for a in inputs for i in (0, 2)] + [p for m in layers for p in m.parameters()]
    names = ["in%d/%d" % (k, i) for k in range(3) for i in (0, 2)] + \
        ["%d.%s" % (k, n) for k, m in enumerate(layers) for n, _ in m.named_parameters()]
    return dict(zip(names, torch.autograd.grad(loss, leaves)))


def test_modules_under_inductor_match_eager_without_breaks_or_recompiles():
    layers = _layers()
    cnt = CompileCounterWithBackend("inductor")
    compiled = torch.compile(_step, fullgraph=True, backend=cnt)
    gen = torch.Generator().manual_seed(99)
    for ac, tol in ((None, 2e-5), (torch.bfloat16, 1e-2)):
        for it in range(3):                               # three training steps, new inputs and offset tensors each
            inputs = _layer_inputs(it)
            with torch.autocast("cuda", dtype=ac or torch.float32, enabled=ac is not None):
                outs_e = _step(layers, inputs)
                weights = [torch.randn(o.shape, generator=gen).to(DEV) for o in outs_e]
                grads_e = _grads(layers, inputs, outs_e, weights)
                outs_c = compiled(layers, inputs)
                grads_c = _grads(layers, inputs, outs_c, weights)
            for k, (a, b) in enumerate(zip(outs_c, outs_e)):
                assert a.dtype == b.dtype
                err = float((a.float() - b.float()).abs().max())
                assert err <= tol * float(b.float().abs().max()), (ac, it, k, err)
            for name, b in grads_e.items():
                if ac is not None and ("sampling_offsets" in name or name.endswith("/0")):
                    # 16-bit: a sampling position one rounding step away may land in the neighbouring pixel cell; the
                    # gradients through positions then jump (as in test_modules_run_under_autocast_in_16_bit_storage)
                    continue
                err = float((grads_c[name].float() - b.float()).abs().max())
                assert err <= tol * max(1e-6, float(b.float().abs().max())), (ac, it, name, err)
        assert cnt.frame_count == (1 if ac is None else 2), cnt.frame_count       # no recompilation over the steps
    assert not torch._dynamo.utils.counters["graph_break"]


def test_export_of_msdeformattn_runs_the_kernels():
    from devis_amd.modules import MSDeformAttn
    layer = _layers()[0].eval()
    assert isinstance(layer, MSDeformAttn)
    args = tuple(a.detach() if a.is_floating_point() else a for a in _layer_inputs(3)[0])
    ep = torch.export.export(layer, args)
    assert "devis_amd.ms_deform_attn_forward" in str(ep.graph)
    with torch.no_grad():
        got, want = ep.module()(*args)[0], layer(*args)[0]
    assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))


def test_path_b_reference_function_under_inductor_is_bit_identical():
    from test_dropin import _reference_shaped_function
    sys.path.insert(0, os.path.join(ROOT, "integration"))
    try:
        sys.modules.pop("MultiScaleDeformableAttention", None)
        fn = _reference_shaped_function(importlib.import_module("MultiScaleDeformableAttention"))
        d = make_inputs(13, N=2, M=8, D=32, Lq=300, shapes=PYR_A, P=4)
        t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
        call = lambda v, ss, lsi, l, a: fn.apply(v, ss, lsi, l, a, 64)
        res, _ = _eager_and_compiled(call, [t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"]], (0, 3, 4), t["grad_out"])
        _assert_same_as_eager(res)
        assert not torch._dynamo.utils.counters["graph_break"]
    finally:
        sys.path.remove(os.path.join(ROOT, "integration"))
        sys.modules.pop("MultiScaleDeformableAttention", None)

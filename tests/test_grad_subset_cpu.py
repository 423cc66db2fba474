"""Which gradients the backward computes (grads mask), on the oracle-backed CPU double of the two bindings
(msda_backward_grads / msda_temporal_backward_grads) in tests/fake_native.py: no GPU needed."""
import numpy as np
import pytest
import torch

import fake_native
from helpers import make_inputs, make_temporal_inputs

VALUE, SAMPLING = 1, 2


@pytest.fixture
def calls(monkeypatch):
    """tests/fake_native.py, recording (binding, grads) of every backward call."""
    seen = []
    fake_native.install(monkeypatch, calls=seen)
    return seen


def _plain(dtype=torch.float64):
    d = make_inputs(11, N=2, M=2, D=8, Lq=5, shapes=[(6, 4), (3, 2)], P=2)
    return {k: torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in d.items()}


def _temporal(dtype=torch.float64):
    d = make_temporal_inputs(12, T=3, W=2, M=2, D=8, Lq=5, shapes=[(6, 4), (3, 2)], Pc=2, Pt=2)
    return {k: torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in d.items()}


SUBSETS = [(v, l, a) for v in (0, 1) for l in (0, 1) for a in (0, 1) if v or l or a]


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "v%dl%da%d" % s)
def test_plain_function_reaches_the_binding_and_mask_its_needs_give(calls, subset):
    from devis_amd.functions import MSDeformAttnFunction
    t = _plain()
    leaves = [t[k].clone().requires_grad_(bool(s)) for k, s in zip(("value", "loc", "aw"), subset)]
    out = MSDeformAttnFunction.apply(leaves[0], t["shapes"], t["lsi"], leaves[1], leaves[2], 1)
    got = out.grad_fn.apply(t["grad_out"])
    want = (VALUE if subset[0] else 0) | (SAMPLING if subset[1] or subset[2] else 0)
    assert calls == [("backward_grads", want)] * 2      # im2col_step 1, N = 2
    for g, s in zip((got[0], got[3], got[4]), subset):
        assert (g is not None) == bool(s)
    # the gradients that are computed are the full backward's
    full = [t[k].clone().requires_grad_(True) for k in ("value", "loc", "aw")]
    ref = torch.autograd.grad(MSDeformAttnFunction.apply(full[0], t["shapes"], t["lsi"], full[1], full[2], 1), full,
                              t["grad_out"])
    for g, r, s in zip((got[0], got[3], got[4]), ref, subset):
        if s:
            assert torch.equal(g, r)


@pytest.mark.parametrize("subset", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)], ids=str)
def test_temporal_function_reaches_the_binding_and_mask_its_needs_give(calls, subset):
    from devis_amd.functions import MSDeformAttnTemporalFunction
    t = _temporal()
    v = t["value"].clone().requires_grad_(bool(subset[0]))
    lc, lt = (t[k].clone().requires_grad_(bool(subset[1])) for k in ("loc_c", "loc_t"))
    ac, at = (t[k].clone().requires_grad_(bool(subset[2])) for k in ("aw_c", "aw_t"))
    out = MSDeformAttnTemporalFunction.apply(v, t["shapes"], t["lsi"], t["ftab"], lc, ac, lt, at, 1)
    got = out.grad_fn.apply(t["grad_out"])
    want = (VALUE if subset[0] else 0) | (SAMPLING if subset[1] or subset[2] else 0)
    assert calls == [("temporal_backward_grads", want)]
    assert (got[0] is not None) == bool(subset[0])
    for g, s in zip(got[4:8], (subset[1], subset[2], subset[1], subset[2])):
        assert (g is not None) == bool(s)


def test_only_the_temporal_locations_need_grad():
    """The mask follows any of the four sampling inputs."""
    from devis_amd.functions import ms_deform_attn_func as F
    assert F._grads_mask(False, False, False, True, False) == SAMPLING
    assert F._grads_mask(True, False, False, False, False) == VALUE
    assert F._grads_mask(False, False, False, False, False) == 0


def test_opcheck_of_the_two_grads_ops(calls):
    from devis_amd import ops
    t = _plain(torch.float32)
    for grads in (VALUE, SAMPLING):
        torch.library.opcheck(ops.ms_deform_attn_backward_grads,
                              (t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], 1, grads))
    tt = _temporal(torch.float32)
    for grads in (VALUE, SAMPLING):
        torch.library.opcheck(ops.temporal_backward_grads,
                              (tt["value"], tt["shapes"], tt["lsi"], tt["ftab"], tt["loc_c"], tt["aw_c"], tt["loc_t"],
                               tt["aw_t"], tt["grad_out"], 1, grads))
    gv, gl, ga = ops.ms_deform_attn_backward_grads(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], 1,
                                                   SAMPLING)
    assert gv.numel() == 0 and gl.shape == t["loc"].shape and ga.shape == t["aw"].shape


@pytest.mark.parametrize("frozen", ["value_side", "sampling_side"])
def test_compiled_module_with_frozen_parameters_matches_eager(calls, frozen):
    """aot_eager compiles the autograd formulas of the forward ops: a partial mask must reach the grads op there too."""
    from devis_amd.modules import MSDeformAttn
    torch.manual_seed(0)
    shapes = torch.tensor([[6, 4], [3, 2]], dtype=torch.int64)
    lsi = torch.tensor([0, 24], dtype=torch.int64)
    mod = MSDeformAttn(d_model=16, n_levels=2, n_heads=2, n_points=2)
    for k, p in mod.named_parameters():
        if (frozen == "value_side") == ("value_proj" in k):
            p.requires_grad_(False)
    query, ref, src = torch.randn(1, 5, 16), torch.rand(1, 5, 2, 2), torch.randn(1, 30, 16)
    query.requires_grad_(frozen == "value_side")
    src.requires_grad_(frozen == "sampling_side")
    ps = [p for _, p in sorted(mod.named_parameters()) if p.requires_grad]
    eager = torch.autograd.grad(mod(query, ref, src, shapes, lsi, None)[0].square().sum(), ps)
    eager_calls = list(calls)
    del calls[:]
    torch._dynamo.reset()
    got = torch.autograd.grad(torch.compile(mod, backend="aot_eager", fullgraph=True)(query, ref, src, shapes, lsi, None)[0]
                              .square().sum(), ps)
    want = SAMPLING if frozen == "value_side" else VALUE
    assert eager_calls and {c[1] for c in eager_calls} == {want}
    assert calls and {c[1] for c in calls} == {want}
    for a, b in zip(got, eager):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)

"""torch.use_deterministic_algorithms(True) on the host side (no GPU): the Functions and ops hand the library
MSDA_GRAD_DETERMINISTIC exactly when the flag is set and grad_value is asked for, the binding then sizes the workspace with
msda_backward_workspace_bytes_det, and the custom ops still pass opcheck.  The library is stood in for by the oracle-backed
tests/fake_native.py, which records every call of the two grads bindings."""
import contextlib

import pytest
import torch

import fake_native
from helpers import make_inputs, make_temporal_inputs

VALUE, SAMPLING, ALL, DET = 1, 2, 3, 4


@pytest.fixture
def flag():
    """Restores the deterministic-algorithms setting the test changes."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


@pytest.fixture
def calls(monkeypatch):
    """tests/fake_native.py, recording (binding, grads) of every backward call."""
    seen = []
    fake_native.install(monkeypatch, calls=seen)
    return seen


def _plain(dtype=torch.float64):
    d = make_inputs(21, N=2, M=2, D=8, Lq=5, shapes=[(6, 4), (3, 2)], P=2)
    return {k: torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in d.items()}


def _temporal(dtype=torch.float64):
    d = make_temporal_inputs(22, T=3, W=2, M=2, D=8, Lq=5, shapes=[(6, 4), (3, 2)], Pc=2, Pt=2)
    return {k: torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in d.items()}


def _plain_backward(t, leaves=("value", "loc", "aw")):
    from devis_amd.functions import MSDeformAttnFunction
    ins = {k: t[k].clone().requires_grad_(k in leaves) for k in ("value", "loc", "aw")}
    out = MSDeformAttnFunction.apply(ins["value"], t["shapes"], t["lsi"], ins["loc"], ins["aw"], 1)
    return torch.autograd.grad(out, [ins[k] for k in leaves], t["grad_out"])


def _temporal_backward(t):
    from devis_amd.functions import MSDeformAttnTemporalFunction
    names = ("value", "loc_c", "aw_c", "loc_t", "aw_t")
    ins = [t[k].clone().requires_grad_(True) for k in names]
    out = MSDeformAttnTemporalFunction.apply(ins[0], t["shapes"], t["lsi"], t["ftab"], *ins[1:], 1)
    return torch.autograd.grad(out, ins, t["grad_out"])


@pytest.mark.parametrize("mode", ["off", "on", "warn_only"])
def test_plain_function_passes_the_bit_iff_the_flag_is_set(calls, flag, mode):
    torch.use_deterministic_algorithms(mode != "off", warn_only=mode == "warn_only")
    t = _plain()
    got = _plain_backward(t)
    assert calls == [("backward_grads", ALL if mode == "off" else ALL | DET)] * 2      # im2col_step 1, N = 2
    torch.use_deterministic_algorithms(False)
    ref = _plain_backward(t)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["off", "on", "warn_only"])
def test_temporal_function_passes_the_bit_iff_the_flag_is_set(calls, flag, mode):
    torch.use_deterministic_algorithms(mode != "off", warn_only=mode == "warn_only")
    _temporal_backward(_temporal())
    assert calls == [("temporal_backward_grads", ALL if mode == "off" else ALL | DET)]


def test_no_bit_without_grad_value(calls, flag):
    """grad_loc / grad_aw are atomic-free on every route: a backward that does not ask for grad_value is unchanged."""
    torch.use_deterministic_algorithms(True)
    _plain_backward(_plain(), leaves=("loc", "aw"))
    assert calls == [("backward_grads", SAMPLING)] * 2
    calls.clear()
    _plain_backward(_plain(), leaves=("value",))
    assert calls == [("backward_grads", VALUE | DET)] * 2


class _FakeLib:
    """Stands in for the loaded library inside the binding: records the workspace queries and the grads calls."""

    def __init__(self):
        self.log = []

    def msda_backward_workspace_bytes(self, *a):
        self.log.append(("ws", a))
        return 1000

    def msda_backward_workspace_bytes_det(self, *a):
        self.log.append(("ws_det", a))
        return 4096

    def msda_backward_grads(self, grads, *a):
        self.log.append(("backward_grads", grads, a[-4]))        # (the workspace byte count)
        return 0

    def msda_temporal_backward_grads(self, grads, *a):
        self.log.append(("temporal_backward_grads", grads, a[-4]))
        return 0


@pytest.fixture
def fake_lib(monkeypatch):
    from devis_amd import _native
    lib = _FakeLib()
    monkeypatch.setattr(_native, "load", lambda: lib)
    monkeypatch.setattr(_native, "_on", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(_native, "_stream", lambda t: None)
    monkeypatch.setattr(_native, "shapes_hint", lambda shapes: None)
    return lib


def test_binding_sizes_the_workspace_with_the_deterministic_query(fake_lib):
    from devis_amd import _native
    t = _plain(torch.float32)
    gv = torch.empty(t["value"].shape)
    gl, ga = torch.empty_like(t["loc"]), torch.empty_like(t["aw"])
    _native.backward_grads(ALL | DET, t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], gv, gl, ga)
    N, S, M, D = t["value"].shape
    assert fake_lib.log == [("ws_det", (N, 1, S, M, D)), ("backward_grads", ALL | DET, 4096)]
    fake_lib.log.clear()
    _native.backward_grads(ALL, t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], gv, gl, ga)
    assert [e[0] for e in fake_lib.log] == ["ws", "backward_grads"] and fake_lib.log[1][1:] == (ALL, 1000)

    fake_lib.log.clear()
    tt = _temporal(torch.float32)
    G, S, M, D = tt["value"].shape
    outs = [torch.empty(tt["value"].shape)] + [torch.empty_like(tt[k]) for k in ("loc_c", "aw_c", "loc_t", "aw_t")]
    _native.temporal_backward_grads(VALUE | DET, tt["value"], tt["shapes"], tt["lsi"], tt["ftab"], tt["loc_c"], tt["aw_c"],
                                    tt["loc_t"], tt["aw_t"], tt["grad_out"], 1, *outs)
    assert fake_lib.log == [("ws_det", (1, G, S, M, D)), ("temporal_backward_grads", VALUE | DET, 4096)]


def test_full_backward_wrappers_delegate_to_the_grads_bindings(fake_lib):
    """_native.backward / temporal_backward (the benchmark's, the tuner's and the scripts' entry points) are the grads
    bindings with GRAD_ALL: one library call each, the workspace queried when none is given, else the caller's taken as it
    is -- as a keyword and as the 16th positional argument."""
    from devis_amd import _native
    t = _plain(torch.float32)
    gv = torch.empty(t["value"].shape)
    gl, ga = torch.empty_like(t["loc"]), torch.empty_like(t["aw"])
    _native.backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], gv, gl, ga)
    N, S, M, D = t["value"].shape
    Lq, L = t["loc"].shape[1], t["loc"].shape[3]
    assert fake_lib.log == [("ws", (N, Lq, M, L)), ("backward_grads", ALL, 1000)]

    tt = _temporal(torch.float32)
    G, W = tt["value"].shape[0], tt["ftab"].shape[1]
    args = [tt[k] for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")] + [1]
    outs = [torch.empty(tt["value"].shape)] + [torch.empty_like(tt[k]) for k in ("loc_c", "aw_c", "loc_t", "aw_t")]
    fake_lib.log.clear()
    _native.temporal_backward(*args, *outs)
    assert fake_lib.log == [("ws", (G, Lq, M, L * (1 + W))), ("temporal_backward_grads", ALL, 1000)]
    ws = torch.empty(300, dtype=torch.int32)
    fake_lib.log.clear()
    _native.temporal_backward(*args, *outs, workspace=ws)
    _native.temporal_backward(*args, *outs, ws)
    assert fake_lib.log == [("temporal_backward_grads", ALL, 1200)] * 2


def test_full_backward_wrappers_reach_a_replaced_grads_binding(calls):
    """The wrappers look their target up when called: with the grads bindings replaced (here by tests/fake_native.py) a call
    through _native.backward / temporal_backward arrives at the replacement."""
    from devis_amd import _native
    t = _plain()
    outs = [torch.full_like(t[k], float("nan")) for k in ("value", "loc", "aw")]
    _native.backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], *outs)
    tt = _temporal()
    touts = [torch.full_like(tt[k], float("nan")) for k in ("value", "loc_c", "aw_c", "loc_t", "aw_t")]
    _native.temporal_backward(*(tt[k] for k in ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")),
                              1, *touts)
    assert calls == [("backward_grads", ALL), ("temporal_backward_grads", ALL)]
    assert not any(torch.isnan(x).any() for x in outs + touts)


def test_deterministic_symbols_and_bit_are_declared():
    from devis_amd import _native
    assert _native.GRAD_DETERMINISTIC == 4 and _native.MSDA_ABI_VERSION == 14
    assert "msda_backward_workspace_bytes_det" in _native.EXPORTED_SYMBOLS


def test_opcheck_of_the_ops_with_the_flag(calls, flag):
    from devis_amd import ops
    torch.use_deterministic_algorithms(True)
    t = _plain(torch.float32)
    torch.library.opcheck(ops.ms_deform_attn_backward, (t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], 1))
    for grads in (VALUE, SAMPLING):
        torch.library.opcheck(ops.ms_deform_attn_backward_grads,
                              (t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], 1, grads))
    tt = _temporal(torch.float32)
    args = (tt["value"], tt["shapes"], tt["lsi"], tt["ftab"], tt["loc_c"], tt["aw_c"], tt["loc_t"], tt["aw_t"], tt["grad_out"], 1)
    torch.library.opcheck(ops.temporal_backward, args)
    torch.library.opcheck(ops.temporal_backward_grads, args + (VALUE,))
    assert ("backward_grads", ALL | DET) in calls and ("temporal_backward_grads", VALUE | DET) in calls


def test_graphed_signature_carries_the_flag(flag):
    from devis_amd.graphs import GraphedLayer
    layer = GraphedLayer(torch.nn.Identity())
    x = torch.zeros(2)
    torch.use_deterministic_algorithms(False)
    off = layer._signature((x,))
    torch.use_deterministic_algorithms(True)
    on = layer._signature((x,))
    assert off != on


def test_clip_parallel_warns_once_in_deterministic_mode(flag, monkeypatch):
    from devis_amd import clip_parallel
    monkeypatch.setattr(clip_parallel, "_warned_deterministic", False)
    torch.use_deterministic_algorithms(True)
    with pytest.warns(UserWarning, match="not covered"):
        clip_parallel._warn_if_deterministic()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        clip_parallel._warn_if_deterministic()

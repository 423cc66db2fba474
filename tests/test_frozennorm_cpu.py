"""CPU tests of the ResNet glue (include/frozennorm.h): the header against the binding, argument errors
without a GPU, the torch composite and the test stand-in against the fixture recorded from the reference, and -- on the test
double tests/fake_frozennorm.py -- which calls a patched stem and two blocks issue, which gradients the backward asks for, the
fallbacks and the patch bookkeeping.

Tolerances.  Everything here is float64: the bound of tests/frozennorm_oracle.py with u = 2^-53, element by element.  The patched
stand-in against the stock one goes through seven convolutions: 1e-12 of each tensor's maximum (tests/test_prenorm_cpu.py's
kind of bar for float64 against float64)."""
import copy
import ctypes
import os
import re

import pytest
import torch

import fake_frozennorm
import frozennorm_oracle as O
import resnet_cases as R
from conftest import ROOT, golden

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


def close(got, want, what, tol=1e-12):
    err, ref = float((got.detach().double() - want.detach().double()).abs().max()), float(want.detach().abs().max())
    assert got.shape == want.shape and err <= tol * ref, (what, err, ref)


# ---- library -----------------------------------------------------------------------------------------------------------------

def test_library_exports_every_symbol_frozennorm_h_declares_and_versions_agree():
    from devis_amd import _binding, _frozennorm, build
    path = build.build()
    header = open(os.path.join(ROOT, "include", "frozennorm.h")).read()
    declared = set(re.findall(r"\b(frozennorm_[a-z_0-9]+)\s*\(", header.split("#ifndef FROZENNORM_H")[1]))
    assert declared == set(_frozennorm.EXPORTED_SYMBOLS) and len(declared) == 6
    raw = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(raw, name), name
    lib = _frozennorm.load()
    assert lib.frozennorm_version() == _frozennorm.FROZENNORM_ABI_VERSION == int(re.search(r"#define FROZENNORM_ABI_VERSION (\d+)", header).group(1))
    assert dict(re.findall(r"FROZENNORM_(F32|BF16|F16) = (\d)", header)) == {"F32": "0", "BF16": "2", "F16": "3"}
    assert dict(re.findall(r"FROZENNORM_(NCHW|NHWC|NONE|PLAIN|NORMED) = (\d)", header)) == {
        "NCHW": str(_frozennorm.NCHW), "NHWC": str(_frozennorm.NHWC), "NONE": str(_frozennorm.NONE),
        "PLAIN": str(_frozennorm.PLAIN), "NORMED": str(_frozennorm.NORMED)}
    assert ctypes.sizeof(_frozennorm.Shape) == 32 and ctypes.sizeof(_frozennorm.Types) == 12 and ctypes.sizeof(_frozennorm.Norm) == 40
    fields = re.search(r"typedef struct frozennorm_shape \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\b(N|C|H|W|layout|residual|relu)\b(?=[,;])", fields) == [n for n, _ in _frozennorm.Shape._fields_]
    assert [lib.frozennorm_pooled_size(n) for n in (-1, 0, 1, 2, 3, 7, 8, 400, 667)] == [-1, 0, 1, 1, 2, 4, 4, 200, 334]
    assert os.path.join(build.include_dir(), "frozennorm.h") in build._headers()
    assert any(s.endswith("frozennorm.hip") for s in build.sources())
    assert "frozennorm.h" in open(os.path.join(ROOT, "setup.py")).read() and "frozennorm.h" in build.include_dir.__doc__
    assert "_frozennorm" in _binding.__doc__
    source = open(os.path.join(ROOT, "devis_amd", "csrc", "frozennorm.hip")).read()
    assert re.findall(r'#include "([^"]+)"', source) == ["op_common.h", "frozennorm.h"]
    body = source.split("namespace frozennorm")[1]
    assert "atomic" not in body and "__shared__" not in source and "hipMalloc" not in source and "Synchronize" not in source
    report = open(os.path.join(ROOT, "profiles", "frozennorm_resource_usage.txt")).read()
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report)
    assert len(scratch) > 100 and set(scratch) == {"0"} and set(re.findall(r"LDS Size \[bytes/block\]: (\d+)", report)) == {"0"}


def test_frozennorm_argument_errors_without_gpu():
    from devis_amd import _frozennorm
    lib = _frozennorm.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.frozennorm_last_error
    NORMED, PLAIN, NHWC = _frozennorm.NORMED, _frozennorm.PLAIN, _frozennorm.NHWC
    shape = lambda N=2, C=4, H=5, W=7, layout=0, residual=0, relu=1: ctypes.byref(_frozennorm.Shape(N, C, H, W, layout, residual, relu))      # noqa: E731
    types = lambda x=0, r=0, y=0: ctypes.byref(_frozennorm.Types(x, r, y))      # noqa: E731
    norm = lambda w=p, b=p, m=p, v=p, eps=1e-5: ctypes.byref(_frozennorm.Norm(w.value if w else None, b.value if b else None, m.value if m else None, v.value if v else None, eps))      # noqa: E731
    fwd = lambda t=types(), s=shape(), x=p, n=norm(), r=None, nr=None, y=p: lib.frozennorm_forward(t, s, x, n, r, nr, y, None)      # noqa: E731
    bwd = lambda t=types(), s=shape(), gy=p, y=p, n=norm(), nr=None, gx=p, gr=None: lib.frozennorm_backward(t, s, gy, y, n, nr, gx, gr, None)      # noqa: E731
    pool = lambda t=types(), s=shape(), x=p, n=norm(), y=p: lib.frozennorm_pool_forward(t, s, x, n, y, None)      # noqa: E731
    for call in (fwd, bwd, pool):
        assert call(s=None) == -1 and b"null pointer" in err()
        assert call(t=None) == -1 and b"null pointer" in err()
        assert call(s=shape(C=0)) == -1 and b"positive" in err()
        assert call(s=shape(N=-1)) == -1 and b"negative" in err() and call(s=shape(H=-1)) == -1 and b"negative" in err()
        assert call(s=shape(N=1 << 31)) == -1 and b"31 bits" in err()
        assert call(s=shape(layout=2)) == -1 and b"layout" in err()
        assert call(s=shape(residual=3)) == -1 and b"residual form" in err()
        assert call(s=shape(relu=2)) == -1 and b"relu" in err()
        # bad dtypes: float64; a code out of range; bfloat16 beside float16; a residual dtype without a residual
        for bad in (dict(x=1, r=1, y=1), dict(x=9), dict(x=2, r=2, y=3), dict(x=3, r=2, y=0)):
            assert call(t=types(**bad), s=shape(residual=PLAIN)) == -1 and b"dtype" in err(), bad
        assert call(t=types(r=2)) == -1 and b"types.r" in err()
        # every mix of float32 with one 16-bit dtype passes the dtype check (N = 0: nothing is launched)
        for half in (2, 3):
            for x in (0, half):
                for r in (0, half):
                    for y in (0, half):
                        assert call(t=types(x, r, y), s=shape(N=0, residual=PLAIN)) in (0, -1) and b"dtype" not in err(), (x, r, y)
    assert fwd(n=None) == -1 and b"norm is required" in err()
    for missing in ("w", "b", "m", "v"):
        assert fwd(n=norm(**{missing: None})) == -1 and b"buffer" in err(), missing
    assert fwd(n=norm(eps=float("nan"))) == -1 and b"eps" in err()
    assert fwd(y=None) == -1 and fwd(x=None) == -1 and b"null pointer" in err()
    assert fwd(r=p) == -1 and b"without a residual" in err()
    assert fwd(nr=norm()) == -1 and b"norm_r" in err() and fwd(s=shape(residual=PLAIN), r=p, nr=norm()) == -1 and b"norm_r" in err()
    assert fwd(s=shape(residual=PLAIN)) == -1 and b"r is required" in err()
    assert fwd(s=shape(residual=NORMED), r=p) == -1 and b"norm_r is required" in err()
    assert bwd(gx=None) == -1 and b"no gradient" in err()
    assert bwd(gr=p) == -1 and b"grad_r" in err()
    assert bwd(gy=None) == -1 and b"grad_y" in err() and bwd(y=None) == -1 and b"ReLU" in err()
    assert bwd(n=None) == -1 and b"norm is required" in err()
    assert bwd(s=shape(residual=NORMED), gr=p) == -1 and b"norm_r is required" in err()
    assert bwd(n=norm(b=None, m=None), s=shape(N=0)) == 0                                    # a backward reads weight and var alone
    assert pool(s=shape(residual=PLAIN), t=types()) == -1 and b"no residual form" in err()
    assert pool(y=None) == -1 and pool(x=None) == -1 and b"null pointer" in err()
    assert fwd(s=shape(C=1 << 30, layout=NHWC, H=1, W=1, N=1)) == -1 and b"channels" in err()
    # nothing to compute: nothing is launched, nothing is dereferenced
    for empty in (shape(N=0), shape(H=0), shape(W=0), shape(N=0, layout=NHWC)):
        assert fwd(s=empty, x=None) == 0 and bwd(s=empty, gy=None, y=None) == 0 and pool(s=empty, x=None) == 0
    from devis_amd.functions import frozen_norm
    assert [frozen_norm.pooled(n) for n in (0, 1, 2, 7, 8, 667)] == [lib.frozennorm_pooled_size(n) for n in (0, 1, 2, 7, 8, 667)]


# ---- the fixture and the composite -------------------------------------------------------------------------------------------

def test_composite_and_stand_in_reproduce_the_reference_fixture_within_the_float64_bound():
    import devis_amd
    case = {k: torch.from_numpy(v) for k, v in golden("frozennorm").items()}
    x, out = case["x"], case["out"]
    state = {k[len("state/"):]: v for k, v in case.items() if k.startswith("state/")}
    norm = (state["weight"], state["bias"], state["running_mean"], state["running_var"], 1e-5)
    want, E = O.forward(x, norm, u=O.U64)
    O.check(out, want, E, "the fixture against the oracle")
    O.check(devis_amd.frozen_batch_norm(x, *norm[:4]), out, E, "composite")
    O.check(devis_amd.frozen_batch_norm(x.contiguous(memory_format=torch.channels_last), *norm[:4]), out, E, "composite, channels-last")
    stand_in = R.FrozenBatchNorm2d(x.shape[1]).double()
    stand_in.load_state_dict({k: v for k, v in state.items() if k != "num_batches_tracked"})
    O.check(stand_in(x), out, E, "stand-in")
    # the other forms of the composite, and the pool, against the oracle
    r, norm_r = O.random_input(x.shape, 3, F64), O.random_norm(x.shape[1], 4, F64)
    for residual, rn in ((None, None), (r, None), (r, norm_r)):
        for relu in (False, True):
            got = devis_amd.frozen_batch_norm(x, *norm[:4], residual=residual, residual_norm=rn, relu=relu)
            O.check(got, *O.forward(x, norm, residual, rn, relu, u=O.U64), "composite %s %s" % (rn is not None, relu))
    O.check(devis_amd.frozen_batch_norm_relu_pool(x, *norm[:4]), *O.pool(x, norm, u=O.U64), "pool composite")
    assert devis_amd.frozen_batch_norm(x.float(), *(t.float() for t in norm[:4]), out_dtype=BF16).dtype == BF16
    assert devis_amd.frozen_batch_norm(x.to(BF16), *(t.float() for t in norm[:4])).dtype == F32          # stock promotion
    with pytest.raises(RuntimeError, match="residual_norm"):
        devis_amd.frozen_batch_norm(x, *norm[:4], residual_norm=norm_r)
    with pytest.raises(RuntimeError, match="one shape"):
        devis_amd.frozen_batch_norm(x, *norm[:4], residual=x[:1])
    with pytest.raises(RuntimeError, match=r"\[6\]"):
        devis_amd.frozen_batch_norm(x, norm[0][:3], *norm[1:4])


# ---- the patched stand-in on the test double ---------------------------------------------------------------------------------

def models(block=R.Bottleneck, dtype=F64, seed=1):
    stock = R.randomise(R.ResNet(block), seed).to(dtype)
    return stock, copy.deepcopy(stock)


def image(dtype=F64, seed=5):
    return O.random_input((2, 3, 21, 30), seed, F64).to(dtype)


FWD, BWD, POOL = "forward", "backward", "pool"


@pytest.mark.parametrize("getter", [False, True])
def test_patched_stem_and_two_blocks_issue_the_expected_calls_and_equal_the_stock_model(monkeypatch, getter):
    import devis_amd
    calls = fake_frozennorm.install(monkeypatch)
    stock, patched = models()
    for m in (stock, patched):
        m.conv1.weight.requires_grad_(False)          # the reference freezes the stem
    root = R.LayerGetter(patched, {"layer1": "0"}) if getter else patched
    keys = list(root.state_dict())
    previous = devis_amd.patch_resnet_glue(root)
    assert len(previous) == 5 and list(root.state_dict()) == keys
    x = image()
    want = stock(x)
    got = root(x)["0"] if getter else root(x)
    # the stem's pool, then per block bn1 and bn2 with ReLU and the tail: NORMED behind the downsample branch, then PLAIN
    assert calls == [(POOL, 0), (FWD, O.NONE, 1, 0), (FWD, O.NONE, 1, 0), (FWD, O.NORMED, 1, 0),
                     (FWD, O.NONE, 1, 0), (FWD, O.NONE, 1, 0), (FWD, O.PLAIN, 1, 0)]
    close(got, want, "output")
    params = [p for p in patched.parameters() if p.requires_grad]
    del calls[:]
    grads = torch.autograd.grad(got, params, torch.ones_like(got))
    # the backward asks only for the gradients needed: grad_r of the last tail feeds the first block, the first block's input
    # -- the frozen stem's output -- needs none, so its bn1 and downsample get grad_x / grad_r alone where a convolution wants it
    assert calls == [(BWD, O.PLAIN, 1, True, True), (BWD, O.NONE, 1, True, False), (BWD, O.NONE, 1, True, False),
                     (BWD, O.NORMED, 1, True, True), (BWD, O.NONE, 1, True, False), (BWD, O.NONE, 1, True, False)]
    for g, w, p in zip(grads, torch.autograd.grad(want, [q for q in stock.parameters() if q.requires_grad], torch.ones_like(want)), params):
        close(g, w, "gradient %s" % (tuple(p.shape),), 1e-11)
    devis_amd.unpatch_resnet_glue(root, previous)
    assert [type(m) for m in patched.modules()] == [type(m) for m in stock.modules()]
    del calls[:]
    close(root(x)["0"] if getter else root(x), want, "unpatched output", 0.0)
    assert calls == []


def test_backward_computes_only_the_gradients_asked_for(monkeypatch):
    import devis_amd
    calls = fake_frozennorm.install(monkeypatch)
    norm, norm_r = O.random_norm(4, 1, F64), O.random_norm(4, 2, F64)
    for want_x, want_r in ((True, False), (False, True), (True, True)):
        x = O.random_input((2, 4, 3, 5), 3, F64).requires_grad_(want_x)
        r = O.random_input((2, 4, 3, 5), 4, F64).requires_grad_(want_r)
        del calls[:]
        y = devis_amd.frozen_batch_norm(x, *norm[:4], residual=r, residual_norm=norm_r, relu=True)
        go = O.random_input(y.shape, 5, F64)
        grads = torch.autograd.grad(y, [t for t in (x, r) if t.requires_grad], go)
        assert calls == [(FWD, O.NORMED, 1, 0), (BWD, O.NORMED, 1, want_x, want_r)]
        (gx, _), (gr, _) = O.backward(go, y, norm, O.NORMED, norm_r, True)
        for g, w in zip(grads, [v for v, on in ((gx, want_x), (gr, want_r)) if on]):
            close(g, w, "gradient")
    # no gradient needed: no Function, no backward; the pool with a gradient wanted: the composite
    del calls[:]
    x = O.random_input((2, 4, 3, 5), 3, F64)
    assert devis_amd.frozen_batch_norm(x, *norm[:4]).grad_fn is None and calls == [(FWD, O.NONE, 0, 0)]
    del calls[:]
    y = devis_amd.frozen_batch_norm_relu_pool(x.requires_grad_(True), *norm[:4])
    assert calls == [] and y.requires_grad
    with torch.no_grad():
        devis_amd.frozen_batch_norm_relu_pool(x, *norm[:4])
    assert calls == [(POOL, 0)]
    # channels-last operands take the channels-last kernels; mixed layouts take the composite
    del calls[:]
    xl = x.detach().contiguous(memory_format=torch.channels_last)
    y = devis_amd.frozen_batch_norm(xl, *norm[:4], residual=xl, relu=True)
    assert calls == [(FWD, O.PLAIN, 1, 1)] and y.is_contiguous(memory_format=torch.channels_last)
    del calls[:]
    devis_amd.frozen_batch_norm(xl, *norm[:4], residual=x.detach())
    devis_amd.frozen_batch_norm(x.detach()[:, :, ::2], *(t for t in norm[:4]))
    assert calls == []


def test_each_fallback_condition_reaches_the_replaced_forward(monkeypatch):
    import devis_amd
    from devis_amd.functions import frozen_norm
    calls = fake_frozennorm.install(monkeypatch)
    stock, patched = models()
    patched.conv1.weight.requires_grad_(False)        # (a stem whose output needs a gradient is a fallback of its own, below)
    ran = []
    for cls in (R.Bottleneck, R.FrozenBatchNorm2d):
        original = cls.forward
        monkeypatch.setattr(cls, "forward", lambda self, x, _f=original, _n=cls.__name__: (ran.append(_n), _f(self, x))[1])
    devis_amd.patch_resnet_glue(patched)
    x = image()
    want = stock(x)
    del ran[:]

    def run(expect_calls, x=x, model=patched, want=want):
        del calls[:], ran[:]
        got = model(x)
        assert bool(calls) == expect_calls, calls
        # the replaced forwards: both blocks, and every norm through them and through the stem's bn1
        assert (ran.count("Bottleneck"), ran.count("FrozenBatchNorm2d")) == ((0, 0) if expect_calls else (2, 8)), ran
        close(got, want, "output")

    run(True)
    monkeypatch.setattr(frozen_norm, "_on_gpu", lambda t: False)                 # CPU tensors
    run(False)
    monkeypatch.setattr(frozen_norm, "_on_gpu", lambda t: True)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)           # while compiling
    run(False)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: False)
    monkeypatch.setattr(frozen_norm, "DTYPES", (F32, BF16, F16))                # float64
    run(False)
    monkeypatch.setattr(frozen_norm, "DTYPES", (F32, BF16, F16, F64))
    monkeypatch.setattr(frozen_norm, "BUFFER_DTYPES", (F32,))                   # buffers that are not float32
    run(False)
    monkeypatch.setattr(frozen_norm, "BUFFER_DTYPES", (F32, F64))
    run(True)
    # an input that requires grad at the stem: bn1 runs the three stock steps itself, the blocks stay fused
    del calls[:], ran[:]
    close(patched(x.clone().requires_grad_(True)), want, "stem with a gradient")
    assert ran == ["FrozenBatchNorm2d"] and len(calls) == 6 and POOL not in [c[0] for c in calls]
    # a block whose norm is not frozen, and a stem whose pool is another, are left alone
    other = R.ResNet(norm=lambda n: torch.nn.BatchNorm2d(n))
    assert devis_amd.patch_resnet_glue(other) == []
    odd = R.ResNet()
    odd.maxpool = torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    assert len(devis_amd.patch_resnet_glue(odd)) == 2
    # a BasicBlock stage
    stock_b, patched_b = models(R.BasicBlock)
    patched_b.conv1.weight.requires_grad_(False)
    assert len(devis_amd.patch_resnet_glue(patched_b)) == 5
    del calls[:]
    close(patched_b(x), stock_b(x), "basic blocks")
    assert calls == [(POOL, 0), (FWD, O.NONE, 1, 0), (FWD, O.NORMED, 1, 0), (FWD, O.NONE, 1, 0), (FWD, O.PLAIN, 1, 0)]


def test_patch_and_unpatch_restore_classes_state_dict_keys_and_a_checkpoint_loads(monkeypatch):
    import devis_amd
    fake_frozennorm.install(monkeypatch)
    stock, patched = models(seed=3)
    before = [(type(m), m.__dict__.keys() - {"_modules"}) for m in patched.modules()]
    keys, names = list(patched.state_dict()), [n for n, _ in patched.named_parameters()]
    previous = devis_amd.patch_resnet_glue(patched)
    assert devis_amd.patch_resnet_glue(patched) == []                           # nothing left to patch
    assert list(patched.state_dict()) == keys and [n for n, _ in patched.named_parameters()] == names
    assert [type(m).__name__ for m, _ in previous] == ["FusedBottleneck", "FusedBottleneck", "FusedFrozenBatchNorm2d", "FusedReLU", "FusedMaxPool2d"]
    assert all(isinstance(m, cls) for m, cls in previous)
    # a checkpoint of another stock model loads into the patched one, which then computes that model
    donor = R.randomise(R.ResNet(), 9).double()
    patched.load_state_dict(donor.state_dict())
    x = image()
    close(patched(x), donor(x), "after loading a checkpoint")
    twin = copy.deepcopy(patched)                                               # (deepcopy keeps the classes)
    assert [type(m) for m in twin.modules()] == [type(m) for m in patched.modules()]
    devis_amd.unpatch_resnet_glue(patched, previous)
    assert [(type(m), m.__dict__.keys() - {"_modules"}) for m in patched.modules()] == before
    assert all(type(m).forward is type(s).forward for m, s in zip(patched.modules(), stock.modules()))


def test_keep_input_dtype_changes_only_the_dtype_asked_for(monkeypatch):
    import devis_amd
    calls = fake_frozennorm.install(monkeypatch)
    stock, plain = models(dtype=F32)
    kept = copy.deepcopy(plain)
    devis_amd.patch_resnet_glue(plain)
    devis_amd.patch_resnet_glue(kept, keep_input_dtype=True)
    dtypes = []
    for block in list(kept.layer1) + list(plain.layer1):       # convolutions that take any dtype and return bfloat16, as under autocast
        for conv in (block.conv1, block.conv2, block.conv3):
            conv.register_forward_pre_hook(lambda m, a: (a[0].float(),))
            conv.register_forward_hook(lambda m, a, out: out.to(BF16))
    from devis_amd import _frozennorm
    inner = _frozennorm.forward
    monkeypatch.setattr(_frozennorm, "forward", lambda types, *a: (dtypes.append(types), inner(types, *a))[1])
    x = image(F32)
    y_plain = plain(x)
    seen_plain, dtypes[:] = list(dtypes), []
    y_kept = kept(x)
    # stock promotion: every fused output float32; kept: the dtype of the convolution output it reads
    assert [t[2] for t in seen_plain] == [F32] * 6 and y_plain.dtype == F32
    assert [t[2] for t in dtypes] == [BF16] * 6 and y_kept.dtype == BF16
    assert [t[0] for t in dtypes] == [t[0] for t in seen_plain] == [BF16] * 6
    assert [c[:2] for c in calls if c[0] == FWD] == [(FWD, O.NONE), (FWD, O.NONE), (FWD, O.NORMED), (FWD, O.NONE), (FWD, O.NONE), (FWD, O.PLAIN)] * 2
    assert float((y_kept.detach().float() - y_plain.detach()).abs().max()) <= 0.05 * float(y_plain.detach().abs().max())


# ---- documents ---------------------------------------------------------------------------------------------------------------

def test_the_documents_describe_the_operator():
    import devis_amd
    read = lambda name: open(os.path.join(ROOT, name)).read()      # noqa: E731
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 23\. .*ResNet", design, re.M)
    section = design.split("## 23.")[1]
    for phrase in ("fma", "rsqrt", "NCHW", "channels-last", "threshold_backward", "torch.library", "is_compiling", "keep_input_dtype",
                   "residual_norm", "max-pool", "resnetglue_bench", "end-to-end", "bitwise"):
        assert phrase in section, phrase
    assert re.search(r"^#+ Backbone: ResNet frozen BatchNorm glue", integration, re.M)
    part = integration.split("Backbone: ResNet frozen BatchNorm glue")[1]
    for phrase in ("patch_resnet_glue", "unpatch_resnet_glue", "keep_input_dtype", "is_compiling", "float64", "IntermediateLayerGetter", "downsample"):
        assert phrase in part, phrase
    assert "frozen_batch_norm" in readme and "frozennorm.h" in readme and "resnetglue_bench.py" in readme
    assert "frozennorm.h" in devis_amd.__doc__ and "frozen_batch_norm_relu_pool" in devis_amd.__doc__
    for name in ("frozen_batch_norm", "frozen_batch_norm_relu_pool", "patch_resnet_glue", "unpatch_resnet_glue"):
        assert name in devis_amd.__all__ and callable(getattr(devis_amd, name))
    assert os.path.exists(os.path.join(ROOT, "scripts", "resnetglue_bench.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "frozennorm_resource_usage.txt"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "resnetglue_bench.json"))

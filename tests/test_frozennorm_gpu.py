"""GPU tests of the ResNet glue (include/frozennorm.h).  Every result is compared element by element
against the bound of tests/frozennorm_oracle.py (eight float32 roundings per term, plus the store's rounding of a 16-bit
output); the bitwise properties are compared with ``==``.

The patched stand-in (a stem and two Bottlenecks, tests/resnet_cases.py) is compared with the stock stand-in on the same device
tensors, both against the stand-in in float64: the patched model's largest distance may exceed the stock model's by no more
than the oracle's bound of the model's last fused call, evaluated on the float64 model's operands: u = 2^-24 in every mode
(the kernels are float32 under autocast too), plus |y| * 2^-8 where keep_input_dtype stores a bfloat16 output.  A weight
gradient may exceed the stock model's distance by GRADIENT_CALLS * 8 * 2^-24 of the float64 gradient's maximum -- the oracle's
cap once for each of the eight fused calls between a weight and the output -- and, with keep_input_dtype, by another
KEPT_ROUNDINGS * 2^-9 of that maximum: that mode rounds thirteen more tensors to bfloat16 than stock promotion does (seven
fused outputs and the gradients of six of them), each by at most bfloat16's unit roundoff.

Largest distances measured on an MI355X (output maximum 21.0): float32, eval and training alike, stock 5.8e-6, patched 7.1e-6,
bound 1.1e-5; weight gradients (maxima 39 to 206) stock at most 8.0e-5, patched at most 6.5e-5, never more than 3.4e-5 above
stock where 64 * 2^-24 of the maximum allows 1.5e-4 to 7.9e-4.  Under autocast stock 0.248; with keep_input_dtype off patched
0.248 and every weight gradient as far as the stock one to four digits; with it on patched 0.286 (0.038 above stock, bound
0.082), and the weight gradients at most 1.4 % of their maximum above stock (53.4 against 51.4 of 146: the stock autocast
backward is itself that far from float64) where 13 * 2^-9 allows 2.5 %."""
import copy

import pytest
import torch
import torch.nn.functional as Fn

import frozennorm_oracle as O
import resnet_cases as R

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
NCHW, NHWC = 0, 1
MAPS = ((1, 1), (1, 3), (7, 1), (5, 67), (25, 42), (8, 8))
FORMS = (O.NONE, O.PLAIN, O.NORMED)


@pytest.fixture(scope="module")
def dev():
    import devis_amd  # noqa: F401
    return torch.device("cuda:0")


def laid(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == NHWC else t.contiguous()


def on(dev, norm):
    return tuple(t.to(dev) for t in norm[:4]) + (norm[4],)


def operands(shape, form, seed, dev, layout, x_dtype=F32, r_dtype=F32):
    """(x, norm, r, norm_r) on the CPU and the same on the device in ``layout``."""
    C = shape[1]
    x, norm = O.random_input(shape, seed, x_dtype), O.random_norm(C, seed + 1)
    r = O.random_input(shape, seed + 2, r_dtype) if form != O.NONE else None
    norm_r = O.random_norm(C, seed + 3) if form == O.NORMED else None
    cpu = (x, norm, r, norm_r)
    gpu = (laid(x.to(dev), layout), on(dev, norm), None if r is None else laid(r.to(dev), layout), None if norm_r is None else on(dev, norm_r))
    return cpu, gpu


def run(gpu, relu, out_dtype=None, wants=(False, False)):
    """y and the requested gradients for a fixed grad_y, through the public function."""
    import devis_amd
    x, norm, r, norm_r = gpu
    x = x.detach().requires_grad_(wants[0])
    r = None if r is None else r.detach().requires_grad_(wants[1])
    y = devis_amd.frozen_batch_norm(x, *norm[:4], eps=norm[4], residual=r, residual_norm=norm_r, relu=relu, out_dtype=out_dtype)
    if not any(wants):
        return y, None, None, None
    g = torch.Generator().manual_seed(99)
    grad_y = torch.empty_like(y).copy_((2 * torch.rand(*y.shape, generator=g, dtype=F64) - 1).to(y.dtype))
    leaves = [t for t, w in ((x, wants[0]), (r, wants[1])) if w]
    grads = list(torch.autograd.grad(y, leaves, grad_y))
    return y, grad_y, grads.pop(0) if wants[0] else None, grads.pop(0) if wants[1] else None


def check_call(cpu, gpu, form, relu, what, out_dtype=None, subsets=None):
    x, norm, r, norm_r = cpu
    subsets = subsets if subsets is not None else ([(True, False)] if form == O.NONE else [(True, False), (False, True), (True, True)])
    y = run(gpu, relu, out_dtype)[0]
    y_dtype = y.dtype
    want, E = O.forward(x, norm, r, norm_r, relu, y_dtype=y_dtype)
    O.check(y, want, E, what + " y")
    assert y.dtype == (out_dtype or F32) and y.stride() == gpu[0].stride()
    for wants in subsets:
        y2, grad_y, gx, gr = run(gpu, relu, out_dtype, wants)
        assert torch.equal(y2, y)
        (wx, Ex), wr = O.backward(grad_y, y2, norm, form, norm_r, relu, x_dtype=x.dtype, r_dtype=None if r is None else r.dtype)
        assert (gx is not None) == wants[0] and (gr is not None) == wants[1]
        if gx is not None:
            assert gx.dtype == x.dtype
            O.check(gx, wx, Ex, what + " grad_x %s" % (wants,))
        if gr is not None:
            assert gr.dtype == r.dtype
            O.check(gr, wr[0], wr[1], what + " grad_r %s" % (wants,))


# ---- the maps -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,C", [(NCHW, 1), (NCHW, 3), (NCHW, 64), (NHWC, 4), (NHWC, 6), (NHWC, 64), (NHWC, 2048)])
def test_every_map_against_the_oracle_forward_and_backward(dev, layout, C):
    for N in (1, 3):
        for i, (H, W) in enumerate(MAPS):
            cpu, gpu = operands((N, C, H, W), O.NORMED, 100 * N + i, dev, layout)
            check_call(cpu, gpu, O.NORMED, True, "N %d C %d map %dx%d layout %d" % (N, C, H, W, layout), subsets=[(True, True)])


@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_every_operand_form_forward_and_every_subset_of_gradients(dev, form, relu, layout):
    for i, shape in enumerate(((3, 3, 5, 67), (3, 64, 25, 42), (2, 6, 1, 3)) if layout == NCHW else ((3, 6, 5, 67), (3, 64, 25, 42), (2, 4, 1, 3))):
        cpu, gpu = operands(shape, form, 7 + i, dev, layout)
        check_call(cpu, gpu, form, relu, "form %d relu %d shape %s layout %d" % (form, relu, shape, layout))


@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("mix", [(F32, F32, F32), (BF16, None, F32), (BF16, F32, F32), (BF16, BF16, BF16), (F16, F16, F16)])
def test_dtype_mixes_without_a_cast_in_between(dev, mix, layout):
    x_dtype, r_dtype, y_dtype = mix
    for i, shape in enumerate(((2, 6, 5, 67), (2, 64, 25, 42))):
        for form in ((O.NONE,) if r_dtype is None else (O.PLAIN, O.NORMED)):
            cpu, gpu = operands(shape, form, 31 + i, dev, layout, x_dtype, r_dtype or x_dtype)
            assert gpu[0].dtype == x_dtype and (gpu[2] is None or gpu[2].dtype == r_dtype)
            # (the stock autocast mix -- 16-bit x, float32 residual -- promotes to float32 on its own: out_dtype None)
            check_call(cpu, gpu, form, True, "mix %s shape %s form %d" % (mix, shape, form), out_dtype=None if y_dtype == F32 else y_dtype)


# ---- bitwise ------------------------------------------------------------------------------------------------------------------

def shifted(t, layout):
    """The same logical tensor one element off the allocation's alignment."""
    N, C, H, W = t.shape
    flat = torch.empty(t.numel() + 9, dtype=t.dtype, device=t.device)
    if layout == NHWC:
        out = flat[1:1 + t.numel()].view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        out = flat[1:1 + t.numel()].view(N, C, H, W)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0
    return out


@pytest.mark.parametrize("shape", [(3, 64, 25, 42), (2, 8, 5, 67), (2, 5, 7, 9)])
def test_bitwise_properties(dev, shape):
    results = {}
    for layout in (NCHW, NHWC):
        cpu, gpu = operands(shape, O.NORMED, 5, dev, layout)
        y, grad_y, gx, gr = run(gpu, True, None, (True, True))
        again = run(gpu, True, None, (True, True))
        for a, b in zip((y, gx, gr), (again[0], again[2], again[3])):
            assert torch.equal(a, b), "two runs of one call"
        # an image alone against the same image in the batch
        alone = tuple(laid(t[1:2], layout) if isinstance(t, torch.Tensor) else t for t in gpu)
        assert torch.equal(run(alone, True)[0], y[1:2]), "an image alone"
        # operands one element off the 16-byte grid: the per-element path
        off = (shifted(gpu[0], layout), gpu[1], shifted(gpu[2], layout), gpu[3])
        y_off, _, gx_off, gr_off = run(off, True, None, (True, True))
        assert torch.equal(y_off, y) and torch.equal(gx_off, gx) and torch.equal(gr_off, gr), "unaligned operands"
        # a 16-bit y is the float32 y rounded once
        for half in (BF16, F16):
            assert torch.equal(run(gpu, True, half)[0], y.to(half)), "rounded once"
        results[layout] = (y, gx, gr)
    for a, b in zip(results[NCHW], results[NHWC]):
        assert torch.equal(a.contiguous(), b.contiguous()), "NCHW against channels-last"


# ---- special values -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [NCHW, NHWC])
def test_nan_and_infinities_propagate_as_in_the_torch_ops_and_masked_gradients_are_zero(dev, layout):
    import devis_amd
    from devis_amd.functions import frozen_norm
    shape = (2, 8, 7, 9)
    cpu, gpu = operands(shape, O.NONE, 3, dev, layout)
    x, norm = gpu[0].clone(), gpu[1]
    flat = x.view(-1) if layout == NCHW else x.permute(0, 2, 3, 1).reshape(-1)
    flat[::7], flat[1::11], flat[2::13] = float("nan"), float("inf"), float("-inf")
    assert flat.data_ptr() == x.data_ptr() and bool(x.isnan().any())
    want, E = O.forward(x, cpu[1], relu=True)
    for fused, stock in ((devis_amd.frozen_batch_norm(x, *norm[:4], relu=True), frozen_norm.frozen_batch_norm_composite(x, *norm, relu=True)),
                         (devis_amd.frozen_batch_norm_relu_pool(x, *norm[:4]), frozen_norm.frozen_batch_norm_relu_pool_composite(x, *norm))):
        assert bool(fused.isnan().any()) and bool(fused.isinf().any())
        assert torch.equal(fused.isnan(), stock.isnan()) and torch.equal(fused.isinf(), stock.isinf())
        assert torch.equal(fused[fused.isinf()], stock[stock.isinf()])
    O.check(devis_amd.frozen_batch_norm(x, *norm[:4], relu=True), want, E, "special values")
    O.check(devis_amd.frozen_batch_norm_relu_pool(x, *norm[:4]), *O.pool(x, cpu[1]), "special values, pooled")
    # y == 0 and NaN give zero gradient, whatever grad_y holds
    xg = x.detach().requires_grad_(True)
    y = devis_amd.frozen_batch_norm(xg, *norm[:4], relu=True)
    (gx,) = torch.autograd.grad(y, [xg], torch.full_like(y, 3.0))
    dead = (y == 0) | y.isnan()
    assert bool(dead.any()) and bool((y == 0).any()) and bool((gx[dead] == 0).all()) and bool((gx[~dead] != 0).all())


@pytest.mark.parametrize("layout", [NCHW, NHWC])
def test_pool_of_an_all_negative_window_is_zero_and_a_negative_weight_reverses_the_order(dev, layout):
    import devis_amd
    C = 8
    ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    x = laid(-1 - torch.rand(2, C, 7, 9, device=dev), layout)
    assert bool((devis_amd.frozen_batch_norm_relu_pool(x, ones, zeros, zeros, ones) == 0).all())
    # w < 0: the window's SMALLEST x gives the largest value
    y = devis_amd.frozen_batch_norm_relu_pool(x, -ones, zeros, zeros, ones, eps=0.0)
    want = Fn.max_pool2d(-x, 3, 2, 1)
    assert torch.equal(y, want)
    norm = (torch.tensor([-1.5, 2.0, -0.5, 1.0, -2.0, 0.7, -1.0, 1.2]), torch.randn(C), torch.randn(C), torch.rand(C) + 0.5, 1e-5)
    xc = O.random_input((2, C, 7, 9), 17)
    y = devis_amd.frozen_batch_norm_relu_pool(laid(xc.to(dev), layout), *on(dev, norm)[:4])
    O.check(y, *O.pool(xc, norm), "pool with negative weights")


# ---- the pool -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("dtypes", [(F32, None), (BF16, None), (BF16, BF16), (F16, F16)])
def test_pool_against_the_oracle(dev, layout, dtypes):
    import devis_amd
    x_dtype, out_dtype = dtypes
    results = []
    for i, (H, W) in enumerate(((1, 1), (2, 3), (7, 9), (8, 8))):
        for N, C in ((2, 3), (1, 8), (2, 64)):
            x, norm = O.random_input((N, C, H, W), 50 + i, x_dtype), O.random_norm(C, 60 + i)
            xd = laid(x.to(dev), layout)
            y = devis_amd.frozen_batch_norm_relu_pool(xd, *on(dev, norm)[:4], out_dtype=out_dtype)
            assert y.shape == (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and y.dtype == (out_dtype or F32)
            O.check(y, *O.pool(x, norm, y_dtype=y.dtype), "pool %s %s" % ((N, C, H, W), dtypes))
            assert torch.equal(y, devis_amd.frozen_batch_norm_relu_pool(shifted(xd, layout), *on(dev, norm)[:4], out_dtype=out_dtype))
            results.append(y)
    if layout == NHWC:      # NCHW against channels-last, bitwise
        for i, (H, W) in enumerate(((1, 1), (2, 3), (7, 9), (8, 8))):
            for j, (N, C) in enumerate(((2, 3), (1, 8), (2, 64))):
                x, norm = O.random_input((N, C, H, W), 50 + i, x_dtype), O.random_norm(C, 60 + i)
                y = devis_amd.frozen_batch_norm_relu_pool(x.to(dev), *on(dev, norm)[:4], out_dtype=out_dtype)
                assert torch.equal(y.contiguous(), results[3 * i + j].contiguous())


# ---- memory -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [NCHW, NHWC])
def test_outputs_over_stale_memory_are_complete_and_nothing_is_written_outside(dev, layout, monkeypatch):
    import devis_amd
    import stale_memory
    from devis_amd.functions import frozen_norm
    shim = stale_memory.install(monkeypatch, [frozen_norm])
    for shape, x_dtype in (((2, 6, 5, 67), F32), ((2, 64, 25, 42), F32), ((3, 8, 7, 1), BF16), ((1, 3, 1, 1), F16)):
        cpu, gpu = operands(shape, O.NORMED, 9, dev, layout, x_dtype, x_dtype)
        y, grad_y, gx, gr = run(gpu, True, None, (True, True))
        want, E = O.forward(*cpu, True, y_dtype=y.dtype)
        O.check(y, want, E, "y over stale memory")
        (wx, Ex), (wr, Er) = O.backward(grad_y, y, cpu[1], O.NORMED, cpu[3], True, x_dtype=x_dtype, r_dtype=x_dtype)
        O.check(gx, wx, Ex, "grad_x over stale memory")
        O.check(gr, wr, Er, "grad_r over stale memory")
        p = devis_amd.frozen_batch_norm_relu_pool(gpu[0], *gpu[1][:4])
        O.check(p, *O.pool(cpu[0], cpu[1]), "pool over stale memory")
    assert len(shim.buffers) == 16 and shim.guards_intact()


# ---- the patched stand-in -----------------------------------------------------------------------------------------------------

GRADIENT_CALLS = 8         # fused calls between a weight and the output, forward and backward: the stem's and seven in the blocks
KEPT_ROUNDINGS = 13        # bfloat16 tensors keep_input_dtype adds: seven fused outputs, and the gradients of the six in the blocks


def _distances(model, x, autocast, train):
    """(output, gradients of the convolution weights) of one forward (and backward)."""
    model.train(train)
    xs = x.to(next(model.parameters()).device, next(model.parameters()).dtype)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        y = model(xs)
    grads = []
    if train:
        g = torch.Generator().manual_seed(4)
        go = torch.randn(y.shape, generator=g, dtype=F64)
        params = [p for n, p in model.named_parameters() if not n.startswith("conv1.")]      # (the stem is frozen)
        grads = torch.autograd.grad(y, params, go.to(y.device, y.dtype))
    return y, grads


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("mode", ["float32", "autocast", "autocast_keep_input_dtype"])
def test_patched_stand_in_is_no_further_from_float64_than_the_stock_one(dev, mode, train):
    import devis_amd
    from devis_amd.modules import resnet_glue
    autocast = mode != "float32"
    stock = R.randomise(R.ResNet(), 2)
    stock.conv1.weight.requires_grad_(False)
    ref = copy.deepcopy(stock).double()
    x = O.random_input((2, 3, 37, 50), 8, F64)
    stock = stock.to(dev)
    patched = copy.deepcopy(stock)
    previous = devis_amd.patch_resnet_glue(patched, keep_input_dtype=mode.endswith("keep_input_dtype"))
    assert len(previous) == 5
    want_y, want_g = _distances(ref, x, False, train)
    got_s, got_p = _distances(stock, x, autocast, train), _distances(patched, x, autocast, train)
    assert got_p[0].dtype == (BF16 if mode.endswith("keep_input_dtype") else F32) and got_s[0].dtype == F32
    # the oracle's bound of the last fused call, on the float64 model's operands
    block, feats = ref.layer1[1], {}
    hooks = [block.register_forward_hook(lambda m, a, o: feats.update(x=a[0])),
             block.conv3.register_forward_hook(lambda m, a, o: feats.update(out=o))]
    with torch.no_grad():
        ref(x)
    for h in hooks:
        h.remove()
    keep = mode.endswith("keep_input_dtype")
    E = O.forward(feats["out"], resnet_glue.norm_of(block.bn3), feats["x"], None, True, u=O.U32, y_dtype=got_p[0].dtype)[1]
    slack = float(E.max())
    dist = lambda a, b: float((a.detach().double().cpu() - b.detach()).abs().max())      # noqa: E731
    d_stock, d_patched = dist(got_s[0], want_y), dist(got_p[0], want_y)
    print("resnet glue %s train=%s: output max %.3e, stock %.3e, patched %.3e, bound %.3e" % (mode, train, float(want_y.abs().max()), d_stock, d_patched, slack))
    assert d_patched <= d_stock + slack
    for gs, gp, gw in zip(got_s[1], got_p[1], want_g):
        ref_max = float(gw.abs().max())
        ds, dp = dist(gs, gw), dist(gp, gw)
        allowed = GRADIENT_CALLS * 8 * O.U32 * ref_max + (KEPT_ROUNDINGS * 2.0 ** -9 * ref_max if keep else 0.0)
        print("    gradient %s: max %.3e, stock %.3e, patched %.3e, allowed above stock %.3e" % (tuple(gw.shape), ref_max, ds, dp, allowed))
        assert dp <= ds + allowed
    devis_amd.unpatch_resnet_glue(patched, previous)
    assert all(type(a) is type(b) for a, b in zip(patched.modules(), stock.modules()))

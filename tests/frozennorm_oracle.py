"""The formula of include/frozennorm.h in float64 (tests only), with the error bound of every element.

    s = w / sqrt(rv + eps)      t = b - rm * s      y = act(x * s1 + t1 + R)

``E = 8 * u * (|x * s1| + |rm1 * s1| + |b1| + |r * s2| + |rm2 * s2| + |b2|)``; for a plain residual ``|r|`` stands for the second
group.  ``u`` is the unit roundoff of the arithmetic under test: 2^-24 for the float32 kernels, 2^-53 for the float64
composite.  The factor 8 is a cap: no term goes through more than eight float32 roundings in ``s`` (an add, a square root, a
division, a product), ``t`` (a product, a subtraction), the fma and the add.  A 16-bit ``y`` adds ``|y| * 2^-8`` (bfloat16) or
``|y| * 2^-11`` (float16): the one rounding at the store.  16-bit inputs enter as the values they hold.  The pool's bound is the
maximum of ``E`` over the window.  The backward takes its mask from the ``y`` it is given -- the kernel's own -- so no element is
left out of a comparison; a gradient is one or two products of ``g`` with a scale of at most four roundings, bounded by the
same cap: ``8 * u * |grad|``, plus the store's rounding for a 16-bit gradient -- relative as above, but at least 2^-25 for
float16, half a step of its subnormals: a gradient is a product and can be that small, where ``E`` has nothing to cover it.

Tensors are logical [N, C, H, W] of any strides; a norm is ``(weight, bias, running_mean, running_var, eps)``."""
import torch
import torch.nn.functional as F

U32, U64 = 2.0 ** -24, 2.0 ** -53
STORE = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL = {torch.float16: 2.0 ** -25}      # half the spacing of float16's subnormals (2^-24), below 2^-14
NONE, PLAIN, NORMED = 0, 1, 2


def constants(norm):
    """(s, t, |rm * s| + |b|) of a norm, each [1, C, 1, 1] float64."""
    w, b, rm, rv = (v.detach().double().cpu().view(1, -1, 1, 1) for v in norm[:4])
    s = w / torch.sqrt(rv + float(norm[4]))
    return s, b - rm * s, (rm * s).abs() + b.abs()


def forward(x, norm, r=None, norm_r=None, relu=False, u=U32, y_dtype=None):
    """(y, E), float64."""
    x = x.detach().double().cpu()
    s1, t1, m1 = constants(norm)
    z, E = x * s1 + t1, (x * s1).abs() + m1
    if r is not None:
        r = r.detach().double().cpu()
        if norm_r is None:
            z, E = z + r, E + r.abs()
        else:
            s2, t2, m2 = constants(norm_r)
            z, E = z + (r * s2 + t2), E + (r * s2).abs() + m2
    y = torch.relu(z) if relu else z
    E = 8 * u * E
    if y_dtype in STORE:
        E = E + y.abs() * STORE[y_dtype]
    return y, E


def pool(x, norm, u=U32, y_dtype=None):
    """(y, E) of max_pool2d(relu(norm(x)), 3, 2, 1)."""
    full, E = forward(x, norm, relu=True, u=u)
    y = F.max_pool2d(full, 3, 2, 1)
    E = F.max_pool2d(torch.nan_to_num(E, nan=float("inf")), 3, 2, 1)
    if y_dtype in STORE:
        E = E + y.abs() * STORE[y_dtype]
    return y, E


def backward(grad_y, y, norm, form=NONE, norm_r=None, relu=False, u=U32, x_dtype=None, r_dtype=None):
    """((grad_x, E_x), (grad_r, E_r) or None); ``y`` is the forward's own output (read behind a ReLU only)."""
    g = grad_y.detach().double().cpu()
    if relu:
        g = torch.where(y.detach().double().cpu() > 0, g, torch.zeros_like(g))

    def bounded(v, dtype):
        E = 8 * u * v.abs()
        if dtype in STORE:          # (relative for a normal number, half a subnormal step for a smaller one)
            E = E + torch.clamp(v.abs() * STORE[dtype], min=SUBNORMAL.get(dtype, 0.0))
        return v, E

    grad_x = bounded(g * constants(norm)[0], x_dtype)
    if form == NONE:
        return grad_x, None
    return grad_x, bounded(g if form == PLAIN else g * constants(norm_r)[0], r_dtype)


def within(got, want, E):
    """Elementwise: equal (infinities included), both NaN, or no further apart than the bound."""
    got = got.detach().double().cpu()
    same = (got == want) | (got.isnan() & want.isnan())
    return same | ((got - want).abs() <= E)


def check(got, want, E, what):
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    ok = within(got, want, E)
    if not bool(ok.all()):
        bad = (~ok).nonzero()[0].tolist()
        at = tuple(bad)
        raise AssertionError("%s: %d elements outside the bound, first at %s: got %r, want %r, bound %r"
                             % (what, int((~ok).sum()), at, float(got[at]), float(want[at]), float(E[at])))


def random_norm(C, seed, dtype=torch.float32):
    """Buffers as the tests draw them: weights of both signs, variances in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, generator=g, dtype=torch.float64)
    w = torch.where(w.abs() < 0.1, torch.full_like(w, 0.5), w)
    return (w.to(dtype), torch.randn(C, generator=g, dtype=torch.float64).to(dtype),
            torch.randn(C, generator=g, dtype=torch.float64).to(dtype),
            (0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)).to(dtype), 1e-5)


def random_input(shape, seed, dtype=torch.float32):
    """|x| <= 4 (keeps float16 finite)."""
    g = torch.Generator().manual_seed(seed)
    return (8 * torch.rand(*shape, generator=g, dtype=torch.float64) - 4).to(dtype)

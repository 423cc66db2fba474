"""Cases shared by tests/test_selfattn_cpu.py and tests/test_selfattn_gpu.py (tests/ only; a plain module, no fixtures): which
compiled kernel variant of csrc/selfattn.hip a call reaches, operand views of equal values, the explicit case lists of the GPU
tests and a seeded generator of sweep configurations.

The host side of selfattn.hip compiles forward_kernel, backward_q_kernel and backward_kv_kernel once per storage type (float32,
bfloat16, float16) and per CT = ceil(D / 16) in 1 .. 4 -- 36 kernels -- and each takes one of three load / store paths at run
time (per element; 8 / 16-byte stores with per-element chunk loads; 8 / 16-byte everything).  The CPU tests assert from the
lists below that every one of them is reached; the GPU tests run the lists."""
import collections
import math
import random

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
KERNELS = ("forward_kernel", "backward_q_kernel", "backward_kv_kernel")
NAMES = ("out", "grad_q", "grad_k", "grad_v")


# ---- which variant a call reaches ------------------------------------------------------------------------------------------------

def variant_of(D, dtype, aligned_and_quad_strided):
    """(CT, chunk_vec, vec) of a call with head dimension ``D`` in storage type ``dtype``.

    RESTATES csrc/selfattn.hip -- change both sides together:
      * CT: ``dispatch_kernel``, ``switch ((D + 15) / 16)``, per storage type of ``dispatch`` (float64 is refused);
      * vec: the ``const bool vec = aligned16(...) && quads(...)`` expressions of ``selfattn_forward`` and
        ``selfattn_backward`` -- every pointer 16-byte aligned, every operand stride a multiple of 4 elements
        (:func:`aligned_and_quad_strided` restates them on tensors);
      * chunk_vec: ``const bool chunk_vec = pb.vec && (n & 3) == 0`` with ``n = D >> 2`` in each of the three kernels."""
    assert dtype in DTYPES and D % 4 == 0 and 4 <= D <= 64, (D, dtype)
    vec = bool(aligned_and_quad_strided)
    return (D + 15) // 16, vec and (D // 4) % 4 == 0, vec


def aligned_and_quad_strided(q, k, v, *dense):
    """The ``vec`` expression of the host on the operands of a call: q, k and v as views, ``dense`` the tensors that are passed
    without strides (grad_out; the results are fresh allocations, which torch aligns)."""
    pointers = all(t.data_ptr() % 16 == 0 for t in (q, k, v) + tuple(dense))
    return pointers and all(t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 for t in (q, k, v))


def classes():
    """The 24 classes (dtype, CT, whether D admits chunk_vec) a sweep has to reach, the dtype varying fastest."""
    return [(dtype, ct, chunk) for ct in (1, 2, 3, 4) for chunk in (False, True) for dtype in DTYPES]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def make_inputs(L, S, N, H, D, dtype=F32, gain=1.0, seed=0):
    """q ~ gain * randn, k, v and grad_out ~ randn, rounded once to ``dtype``, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    q = (gain * torch.randn(L, N, H * D, generator=g, dtype=torch.float64)).to(dtype)
    k, v = (torch.randn(S, N, H * D, generator=g, dtype=torch.float64).to(dtype) for _ in range(2))
    return q, k, v, torch.randn(L, N, H * D, generator=g, dtype=torch.float64).to(dtype)


def planted_inputs(L, S, N, H, D, dtype, key, boost, seed=0):
    """:func:`make_inputs` with a planted row maximum: channel 0 of every head of q is 4, channel 0 of k is 0 except at key
    ``key``, where it is ``boost * sqrt(D) / 4`` -- key ``key`` gains ``boost`` on the logit of every row of every head."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, go = (torch.randn(rows, N, H * D, generator=g, dtype=torch.float64) for rows in (L, S, S, L))
    q[..., ::D] = 4.0
    k[..., ::D] = 0.0
    k[key, :, ::D] = boost * math.sqrt(D) / 4.0
    return tuple(t.to(dtype) for t in (q, k, v, go))


def cancelling_terms(q, k, v, go, D, p):
    """The size of the terms that cancel in grad_q and grad_k = dS times k or q, dS = P (dP - delta): dP and delta are sums of D
    products of grad_out and v, times the largest q or k; with p == 1 those terms are exactly 0."""
    if p >= 1.0:
        return 0.0
    return float(go.abs().max() * v.abs().max()) * D * float(max(q.abs().max(), k.abs().max()))


def run(q, k, v, grad_out, H, p=0.0, seed=None, wants=(True, True, True)):
    """(out, grad_q, grad_k, grad_v) of the operator on the tensors given; a gradient that is not wanted is None."""
    import devis_amd
    leaves = [t.detach().requires_grad_(want) for t, want in zip((q, k, v), wants)]
    out = devis_amd.multihead_attention(*leaves, H, p=p, seed=seed)
    asked = [t for t in leaves if t.requires_grad]
    grads = iter(torch.autograd.grad(out, asked, grad_out)) if asked else iter(())
    return (out.detach(),) + tuple(next(grads) if want else None for want in wants)


# ---- views -----------------------------------------------------------------------------------------------------------------------
# build(q, k, v, grad_out) -> operands of equal values on the device of the dense ones (broadcast: of the values of batch entry
# 0 in q, k and v); vec(E, dtype): whether the host takes the call as ``vec``, forward and backward alike.

View = collections.namedtuple("View", "build vec")


def _shift(t):
    """``t`` one element into its storage: 4 or 2 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    return flat[1:].view(t.shape)


def _dense(q, k, v, go):
    return q.contiguous(), k.contiguous(), v.contiguous(), go


def _packed(q, k, v, go):
    """q and k as the column halves of one [max(L, S), N, 2E] tensor (the module's single projection when L == S)."""
    (L, N, E), S = q.shape, k.shape[0]
    both = torch.zeros(max(L, S), N, 2 * E, dtype=q.dtype, device=q.device)
    both[:L, :, :E] = q
    both[:S, :, E:] = k
    return both[:L, :, :E], both[:S, :, E:], v, go


def _batch_first(q, k, v, go):
    q, k, v = (t.transpose(0, 1).contiguous().transpose(0, 1) for t in (q, k, v))
    return q, k, v, go


def _shifted(q, k, v, go):
    return _shift(q), _shift(k), _shift(v), _shift(go)


def _padded_rows(q, k, v, go):
    """Rows of E + 3 elements: no stride is a multiple of 4."""
    def pad(t):
        wide = torch.zeros(t.shape[0], t.shape[1], t.shape[2] + 3, dtype=t.dtype, device=t.device)
        wide[..., :t.shape[2]] = t
        return wide[..., :t.shape[2]]
    return pad(q), pad(k), pad(v), go


def _only_v_unaligned(q, k, v, go):
    return q, k, _shift(v), go


def _broadcast(q, k, v, go):
    """Batch entry 0 of q, k and v for every batch entry, with a batch stride of 0."""
    q, k, v = (t[:, :1].contiguous().expand(-1, t.shape[1], -1) for t in (q, k, v))
    return q, k, v, go


VIEWS = collections.OrderedDict([
    ("dense", View(_dense, lambda E, dtype: True)),
    # the k half starts E elements into the tensor: 16-byte aligned unless E * itemsize is not a multiple of 16
    ("packed", View(_packed, lambda E, dtype: E * torch.empty((), dtype=dtype).element_size() % 16 == 0)),
    ("batch_first", View(_batch_first, lambda E, dtype: True)),             # strides (E, rows * E, 1), E % 4 == 0
    ("shifted", View(_shifted, lambda E, dtype: False)),                    # no pointer is aligned
    ("padded_rows", View(_padded_rows, lambda E, dtype: False)),            # batch stride E + 3
    ("only_v_unaligned", View(_only_v_unaligned, lambda E, dtype: False)),  # one operand turns vec off for the whole call
    ("broadcast", View(_broadcast, lambda E, dtype: True)),                 # strides (E, 0, 1)
])


# ---- the explicit cases of tests/test_selfattn_gpu.py ----------------------------------------------------------------------------
DROPOUT_SEED = 20260101

MATRIX_SIZES = [(17, 15), (33, 70)]
MATRIX_F32 = [(L, S, 2, 3, D) for L, S in MATRIX_SIZES for D in range(4, 65, 4)]                  # (L, S, N, H, D)
MATRIX_16 = [(33, 70, 2, 2, D, dtype, p) for dtype in (BF16, F16) for D in (4, 8, 16, 20, 36, 40, 48, 52, 64) for p in (0.0, 0.5)]
VIEW_SHAPE = (33, 21, 2, 3)                                                                       # (L, S, N, H)
VIEW_MATRIX = [(D, dtype) for dtype in DTYPES for D in (4, 16, 20, 40, 48, 64)]
PLANTED_SHAPE = (21, 2, 2, 24)                                                                    # (L, N, H, D)
PLANTED = [(S, dtype, p, last, boost) for S in (33, 65) for dtype in DTYPES for p in (0.0, 0.5) for last in (False, True)
           for boost in (9.0, 60.0)]                                                              # the key is S - 1 or 0
LOPSIDED = [(L, S, 2, 3, 12, p) for L, S in ((1, 300), (300, 1), (16, 257), (257, 16)) for p in (0.0, 0.5)]
SWEEP = range(96)


def oracle_matrix_variants():
    """(kernel, dtype, CT) of every launch of the two head-dimension matrices, which ask for out and all three gradients."""
    cases = [(D, F32) for _, _, _, _, D in MATRIX_F32] + [(D, dtype) for _, _, _, _, D, dtype, _ in MATRIX_16]
    return {(kernel, dtype, variant_of(D, dtype, True)[0]) for D, dtype in cases for kernel in KERNELS}


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
Config = collections.namedtuple("Config", "L S N H D dtype p dropout_seed view")

# D by (CT, D admits chunk_vec): the vector chunk path takes D % 16 == 0 alone, one value in sixteen per CT, and a uniform D
# would reach it in a quarter of the draws
_HEAD_DIMS = {(ct, chunk): [D for D in range(16 * ct - 12, 16 * ct + 1, 4) if (D % 16 == 0) == chunk]
              for ct in (1, 2, 3, 4) for chunk in (False, True)}


def sweep_config(seed):
    """Configuration ``seed`` of the sweep, a function of ``seed`` alone.  Stratified, not uniform over D: the class (dtype, CT,
    D admits chunk_vec) is drawn first, as entry ``seed`` modulo 24 of :func:`classes`, and the view is entry ``seed`` modulo 7
    of ``VIEWS``.  Any 24 consecutive seeds reach every class once, any 7 every view, and -- the dtype being ``seed`` modulo 3,
    coprime to 7 -- any 21 every (dtype, view) pair.  D inside its class, the sizes, p and the dropout seed are drawn from
    ``random.Random(seed)``."""
    rng = random.Random(seed)
    dtype, ct, chunk = classes()[seed % 24]
    D = rng.choice(_HEAD_DIMS[ct, chunk])
    L, S = rng.randint(1, 80), rng.randint(1, 80)
    N, H = rng.randint(1, 3), rng.randint(1, 4)
    p = rng.choice((0.0, 0.1, 0.5))
    dropout_seed = rng.randint(-(1 << 63), (1 << 63) - 1)
    return Config(L, S, N, H, D, dtype, p, dropout_seed, list(VIEWS)[seed % 7])

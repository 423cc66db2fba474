"""Shared helpers for the parity tests (test infrastructure; may import the oracle)."""
import numpy as np
import torch

from oracle import msda_oracle as O

PYR_A = [(45, 80), (23, 40), (12, 20), (6, 10)]        # 360x640 input (DeVIS test size), S = 4820
PYR_B = [(100, 167), (50, 84), (25, 42), (13, 21)]     # 800x1333 input, S = 22223


def make_inputs(seed, N, M, D, Lq, shapes, P, loc_mode="wide", dtype=np.float32, value_scale=0.01):
    """Seeded synthetic inputs, rounded ONCE to `dtype` precision (so every path sees identical
    numbers).  loc_mode: 'unit' = rand in [0,1) (reference test.py), 'wide' = rand*1.4-0.2 (exercises
    the out-of-range rules)."""
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, dtype=np.int64)
    L = shapes.shape[0]
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    value = rng.random((N, S, M, D)) * value_scale
    loc = rng.random((N, Lq, M, L, P, 2))
    if loc_mode == "wide":
        loc = loc * 1.4 - 0.2
    aw = rng.random((N, Lq, M, L, P)) + 1e-5
    aw = aw / aw.sum(axis=(-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M * D))
    return dict(value=value.astype(dtype), shapes=shapes, lsi=O.level_start_index(shapes),
                loc=loc.astype(dtype), aw=aw.astype(dtype), grad_out=grad_out.astype(dtype))


def round_to(arrs, torch_dtype):
    """Round numpy float64 arrays through a torch storage dtype (bf16/f16/f32) and back to float64."""
    out = {}
    for k, v in arrs.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            out[k] = torch.from_numpy(np.asarray(v, dtype=np.float64)).to(torch_dtype).double().numpy()
        else:
            out[k] = v
    return out


def oracle_fwd_bwd(d, dtype=np.float64):
    """Oracle outputs (C restatement) for an input dict in the given arithmetic dtype."""
    v, l, a, g = (np.asarray(d[k], dtype=dtype) for k in ("value", "loc", "aw", "grad_out"))
    out = O.forward(v, d["shapes"], d["lsi"], l, a)
    gv, gl, ga = O.backward(v, d["shapes"], d["lsi"], l, a, g)
    return out, gv, gl, ga


def window_level_starts(lsi, S, W):
    """Level starts of W frames of S rows each stacked along the pixel axis: frame w's levels sit where they sit in one frame,
    w * S rows further on (for a compact pyramid: the cumsum of the tiled shapes, as the reference computes them)."""
    lsi = np.asarray(lsi, dtype=np.int64)
    return np.concatenate([lsi + w * S for w in range(W)]).astype(np.int64)


def temporal_reference(value, shapes, lsi, ftab, loc_c, aw_c, loc_t, aw_t, grad_out=None):
    """Oracle for the fused temporal op = the reference's call pattern (ms_deform_attn.py:325-364):
    per frame t one call on value[t] and one on the `window` frames ftab[t] stacked along the level
    axis with spatial_shapes.repeat(window).  numpy float64 in/out.  value [T,S,M,D] (one clip); the level
    layout `lsi` need not tile [0, S) (see relayout)."""
    T, S, M, D = value.shape
    W = ftab.shape[1]
    t_shapes = np.tile(shapes, (W, 1))
    t_lsi = window_level_starts(lsi, S, W)
    outs, gv = [], np.zeros_like(value)
    gl_c, ga_c, gl_t, ga_t = (np.zeros_like(x) for x in (loc_c, aw_c, loc_t, aw_t))
    for t in range(T):
        stacked = value[ftab[t]].reshape(1, W * S, M, D)
        o1 = O.forward(value[t][None], shapes, lsi, loc_c[t][None], aw_c[t][None])
        o2 = O.forward(stacked, t_shapes, t_lsi, loc_t[t][None], aw_t[t][None])
        outs.append(o1 + o2)
        if grad_out is not None:
            g = grad_out[t][None]
            a, b, c = O.backward(value[t][None], shapes, lsi, loc_c[t][None], aw_c[t][None], g)
            gv[t] += a[0]; gl_c[t] = b[0]; ga_c[t] = c[0]
            a, b, c = O.backward(stacked, t_shapes, t_lsi, loc_t[t][None], aw_t[t][None], g)
            for w, f in enumerate(ftab[t]):                         # index_put-add, repeats accumulate (np.add.at, unbuffered)
                gv[f] += a[0, w * S:(w + 1) * S]
            gl_t[t] = b[0]; ga_t[t] = c[0]
    out = np.concatenate(outs, 0)
    if grad_out is None:
        return out
    return out, gv, gl_c, ga_c, gl_t, ga_t


def make_temporal_inputs(seed, T, W, M, D, Lq, shapes, Pc, Pt, ftab=None, dtype=np.float32):
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, dtype=np.int64)
    L = shapes.shape[0]
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    if ftab is None:   # every other frame, ascending (devis_transformer.py:147-150)
        assert W == T - 1
        ftab = np.array([[f for f in range(T) if f != t] for t in range(T)], dtype=np.int32)
    value = rng.random((T, S, M, D)) * 0.01
    loc_c = rng.random((T, Lq, M, L, Pc, 2)) * 1.4 - 0.2
    loc_t = rng.random((T, Lq, M, W * L, Pt, 2)) * 1.4 - 0.2
    aw = rng.random((T, Lq, M, L * Pc + W * L * Pt)) + 1e-5
    aw = aw / aw.sum(-1, keepdims=True)
    aw_c = aw[..., :L * Pc].reshape(T, Lq, M, L, Pc)
    aw_t = aw[..., L * Pc:].reshape(T, Lq, M, W * L, Pt)
    grad_out = rng.standard_normal((T, Lq, M * D))
    f = lambda x: np.ascontiguousarray(x.astype(dtype))
    return dict(value=f(value), shapes=shapes, lsi=O.level_start_index(shapes), ftab=np.ascontiguousarray(ftab),
                loc_c=f(loc_c), aw_c=f(aw_c), loc_t=f(loc_t), aw_t=f(aw_t), grad_out=f(grad_out))


def pixel_centres(shapes):
    """[S, 2] normalised (x, y) centres of the pixels of a pyramid, in query order (= the encoder's reference points,
    deformable_transformer.py:185-198 with valid_ratios = 1)."""
    out = []
    for h, w in np.asarray(shapes, dtype=np.int64).tolist():
        ys, xs = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
        out.append(np.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    return np.concatenate(out, 0)


def localise(loc, shapes, sigma_px, seed, levels_per_slot=None):
    """Replace sampling locations [..., Lq = S, M, LL, P, 2] by encoder-like ones: the query's own pixel centre plus
    N(0, sigma_px^2) pixels of the sampled level (LL = a multiple of the number of levels: slot-major, level-minor)."""
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, dtype=np.int64)
    L = shapes.shape[0]
    c = pixel_centres(shapes)                                           # [S, 2]
    LL = loc.shape[-3]
    wh = np.stack([shapes[:, 1], shapes[:, 0]], -1).astype(np.float64)  # (W, H) per level
    wh = np.tile(wh, (LL // L, 1))                                      # [LL, 2]
    noise = rng.standard_normal(loc.shape) * sigma_px / wh[:, None, :]
    return (c[:, None, None, None, :] + noise).astype(loc.dtype)


LAYOUTS = ("gaps", "aligned", "tail_gap", "reversed", "shuffled")


def relayout(d, kind, seed):
    """The call of input dict `d` (make_inputs / make_temporal_inputs: a compact pyramid) with `value` moved into a larger pixel
    axis of S' rows and level_start_index to match (include/msda.h: levels in any order, with gaps).  Rows of no level are
    NaN -- no kernel may read them -- and `gap` [S'] marks them.  kind:
      gaps      a gap of 1..70 rows before every level and after the last one (lsi[0] > 0)
      aligned   every level starts on a multiple of 64 rows
      tail_gap  one gap, between levels L-2 and L-1, at least as long as level L-1 (one level: before it)
      reversed  coarse levels first in memory, gaps as for `gaps`
      shuffled  a random level order, gaps of 0..70 rows"""
    assert kind in LAYOUTS, kind
    rng = np.random.default_rng(seed)
    shapes = np.asarray(d["shapes"], dtype=np.int64)
    lsi = np.asarray(d["lsi"], dtype=np.int64)
    hw = shapes[:, 0] * shapes[:, 1]
    L = len(hw)
    assert np.array_equal(lsi, O.level_start_index(shapes)), "relayout starts from a compact layout"
    order = list(range(L))
    if kind == "reversed":
        order = order[::-1]
    elif kind == "shuffled":
        order = [int(i) for i in rng.permutation(L)]
        if L > 1 and order == list(range(L)):
            order = order[1:] + order[:1]
    gap = np.zeros(L + 1, dtype=np.int64)            # gap[i]: rows before the i-th level in memory; gap[L]: after the last
    if kind in ("gaps", "reversed"):
        gap[:] = rng.integers(1, 71, size=L + 1)
    elif kind == "shuffled":
        gap[:] = rng.integers(0, 71, size=L + 1)
    elif kind == "tail_gap":
        gap[L - 1 if L > 1 else 0] = hw[-1] + rng.integers(1, 71)
    new_lsi = np.zeros(L, dtype=np.int64)
    pos = 0
    for i, l in enumerate(order):
        pos += int(gap[i])
        if kind == "aligned":
            pos = -(-pos // 64) * 64
        new_lsi[l] = pos
        pos += int(hw[l])
    S2 = pos + int(gap[L]) if kind != "aligned" else -(-pos // 64) * 64
    value = d["value"]
    out = np.full(value.shape[:1] + (S2,) + value.shape[2:], np.nan, dtype=value.dtype)
    is_gap = np.ones(S2, dtype=bool)
    for l in range(L):
        out[:, new_lsi[l]:new_lsi[l] + hw[l]] = value[:, lsi[l]:lsi[l] + hw[l]]
        is_gap[new_lsi[l]:new_lsi[l] + hw[l]] = False
    r = dict(d)
    r.update(value=out, lsi=new_lsi, gap=is_gap)
    return r


def gaps_zeroed(d):
    """`d` with the gap rows of `value` set to 0 (the oracle's input: it reads no gap row either, and NaN would hide that)."""
    r = dict(d)
    r["value"] = np.where(d["gap"][None, :, None, None], np.zeros((), d["value"].dtype), d["value"])
    return r


def level_rows(x, d):
    """Rows of a [N, S', ...] array that belong to a level, in level order -- the compact layout's rows."""
    shapes, lsi = np.asarray(d["shapes"]), np.asarray(d["lsi"])
    return np.concatenate([x[:, s:s + h * w] for (h, w), s in zip(shapes.tolist(), lsi.tolist())], 1)

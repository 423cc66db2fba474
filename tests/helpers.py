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


PLACEMENTS = ("on_grid", "edges", "nonfinite", "huge", "all_out", "piled", "weights")
POW2 = [(32, 64), (16, 32), (8, 16), (4, 8), (2, 2), (1, 1)]       # power-of-two levels: every placed border coordinate is dyadic
POW2_4 = POW2[:4]                                                   # S = 2720, four levels (decoder- and encoder-shaped calls)
HUGE = (1e30, -1e30, 3e9, -3e9, 65504.0, -65504.0, 1e-45, -0.0)     # the first six are out of range for every level and dtype


def _exact(c, n, whole=None):
    """The placed normalised coordinates `c` on levels of size `n`: the kernels' fp32 `c * n - 0.5` equals the fp64 value (kernel
    and fp64 oracle decide range and cell alike), they survive bf16 / f16 storage where the level is at most 64 wide, and the
    pixel coordinates marked `whole` are integers."""
    c, n = np.asarray(c, np.float64), np.asarray(n, np.float64)
    px = c * n - 0.5
    assert np.array_equal((c.astype(np.float32) * n.astype(np.float32) - np.float32(0.5)).astype(np.float64), px)
    assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
    if n.max() <= 64:
        for t in (torch.bfloat16, torch.float16):
            assert np.array_equal(torch.from_numpy(c).to(t).double().numpy(), c), t
    if whole is not None:
        assert np.array_equal(px[whole], np.round(px[whole]))


def _block_run(rng, Lq, blocks=2):
    """Start of a run of `blocks` whole 64-query blocks (the culling records' block summaries), or None if that is over Lq / 6."""
    if Lq < 6 * 64 * blocks:
        return None
    return 64 * int(rng.integers(0, Lq // 64 - blocks + 1))


def place(d, kind, seed, whole=False):
    """The call of input dict `d` (make_inputs / make_temporal_inputs) with part of its sampling locations and attention weights
    overwritten by values random draws do not produce.  Returns (call, masks): masks["placed"], ["out"], ["zero_w"] map each
    location key ("loc", or "loc_c" and "loc_t") to a bool array over its points [B, Lq, M, LL, P] -- the points written, those of
    them that are outside the range test BY CONSTRUCTION (their grad_loc / grad_attn are exactly 0), and those whose weight is
    exactly 0 (their grad_loc is) -- and masks["levels"], ["frames"], ["call"] name what `all_out` emptied (grad_value exactly 0
    there).  Except for `all_out` at most a third of the queries are touched; the rest stay as drawn.  kind:
      on_grid    x*W - 0.5 and / or y*H - 0.5 exactly integer, over every row and column index of every level
      edges      pixel coordinates in (-1, 0) (bottom / right taps only), in (H-1, H) (top / left taps only), exactly -1 and exactly H
                 (excluded), in every combination of the two axes: map corners with one tap inside included
      nonfinite  NaN, +inf, -inf in x, in y, in both: in one point of a group, in every point of a group, in whole query rows (and,
                 with enough queries, two whole blocks of 64 consecutive queries)
      huge       +-1e30, +-3e9, +-65504 (outside), 1e-45 and -0.0 (inside), in x, in y, in both
      all_out    no point in range for one (query, head) (with enough queries: two blocks of 64 queries), for one level, and for one
                 source frame of a temporal call; whole=True: for the entire call
      piled      every point of a run of consecutive queries in one pixel cell, then in the four cells around one grid corner
      weights    whole queries with weights exactly 0, with negative weights, and with weights that sum to 3
    on_grid and edges take power-of-two level sizes (POW2): their coordinates are dyadic, which _exact asserts."""
    assert kind in PLACEMENTS, kind
    rng = np.random.default_rng(seed)
    shapes = np.asarray(d["shapes"], dtype=np.int64)
    L = len(shapes)
    if kind in ("on_grid", "edges"):
        assert all(int(v) & (int(v) - 1) == 0 for v in shapes.reshape(-1)), "on_grid / edges take power-of-two levels"
    r = dict(d)
    masks = dict(placed={}, out={}, zero_w={}, levels=[], frames=[], call=bool(whole and kind == "all_out"))
    pairs = (("loc", "aw"),) if "loc" in d else (("loc_c", "aw_c"), ("loc_t", "aw_t"))
    level = int(rng.integers(0, L))                                      # all_out: the emptied level and source frame
    frame = int(rng.integers(0, d["ftab"].shape[0])) if "ftab" in d else None
    run = _block_run(rng, d[pairs[0][0]].shape[1])                       # nonfinite, all_out: the same blocks in every location array
    for lk, ak in pairs:
        loc, aw = np.array(d[lk], dtype=np.float64), np.array(d[ak], dtype=np.float64)
        B, Lq, M, LL, P, _ = loc.shape
        H = np.tile(shapes[:, 0], LL // L).astype(np.float64)[:, None]      # [LL, 1]: broadcasts over [B, Lq, M, LL, P]
        W = np.tile(shapes[:, 1], LL // L).astype(np.float64)[:, None]
        full = np.zeros((B, Lq, M, LL, P), dtype=bool)
        nq = max(1, Lq // 3)
        qs = rng.permutation(Lq)[:nq]
        pl, ou, zw = full.copy(), full.copy(), full.copy()
        if kind in ("on_grid", "edges"):
            pl[:, qs] = True
            k = (np.cumsum(pl[:, :, :, :1].reshape(-1)) - 1).reshape(B, Lq, M, 1, P)      # running index of the placed points of a level
            k = np.broadcast_to(k, pl.shape)
            if kind == "on_grid":
                i, j = k % H, (7 * k + 3) % W
                fy, fx = np.where(k // 64 % 4 == 3, 0.25, 0.0), np.where(k // 64 % 4 == 1, 0.25, 0.0)      # (the first 64: both whole)
                h_im, w_im = i + fy, j + fx
                for n in range(LL):                                            # every row and column index, on the integer
                    sel = pl[:, :, :, n]
                    assert set(i[:, :, :, n][sel & (fy[:, :, :, n] == 0)]) == set(range(int(H[n, 0])))
                    assert set(j[:, :, :, n][sel & (fx[:, :, :, n] == 0)]) == set(range(int(W[n, 0])))
                wy, wx = pl & (fy == 0), pl & (fx == 0)
            else:
                combos = np.array([(a, b) for a in range(5) for b in range(5) if (a, b) != (4, 4)])       # 24 of them
                assert pl[:, :, :, 0].sum() >= len(combos)
                ky, kx = combos[k % len(combos), 0], combos[k % len(combos), 1]

                def coord(kk, n):      # 0: in (-1, 0)  1: in (n-1, n)  2: exactly -1  3: exactly n  4: inside, a quarter into a cell
                    inside = (5 * k) % np.maximum(n - 1, 1) + 0.25
                    return np.select([kk == 0, kk == 1, kk == 2, kk == 3], [-0.25 + 0 * n, n - 0.75, -1.0 + 0 * n, n + 0.0], inside)
                h_im, w_im = coord(ky, H), coord(kx, W)
                ou = pl & ((ky == 2) | (ky == 3) | (kx == 2) | (kx == 3))
                wy, wx = pl & (ky >= 2) & (ky <= 3), pl & (kx >= 2) & (kx <= 3)
            cand = np.stack([(w_im + 0.5) / W, (h_im + 0.5) / H], -1)
            Hf, Wf = np.broadcast_to(H, pl.shape), np.broadcast_to(W, pl.shape)
            _exact(cand[..., 1][pl], Hf[pl], wy[pl])
            _exact(cand[..., 0][pl], Wf[pl], wx[pl])
            loc = np.where(pl[..., None], cand, loc)
        elif kind in ("nonfinite", "huge"):
            vals = np.array([np.nan, np.inf, -np.inf] if kind == "nonfinite" else HUGE)
            if kind == "nonfinite":
                if run is not None:                                            # whole query rows: two whole blocks of 64 queries
                    rest = np.array([q for q in rng.permutation(Lq) if not run <= q < run + 128][:nq - 128])
                    rows, qs = np.arange(run, run + 128), rest
                else:
                    rows, qs = qs[:max(1, nq // 3)], qs[max(1, nq // 3):]
                pl[:, rows] = True
                some, groups = qs[:len(qs) // 2], qs[len(qs) // 2:]
                pl[:, some, :, :, 0] = True                                    # one point of every group of these queries
                g = (np.arange(M)[:, None] + np.arange(LL)[None, :]) % 2 == 0
                pl[:, groups] |= g[None, None, :, :, None]                     # every point of half of the groups of these
                ou = pl.copy()
            else:
                pl[:, qs, :, :, ::2] = True
            k = (np.cumsum(pl.reshape(-1)) - 1).reshape(pl.shape)                # running index of the placed points
            v, where = vals[k % len(vals)], (k // len(vals)) % 3              # where: 0 = x, 1 = y, 2 = both
            if kind == "huge":
                ou = pl & (k % len(vals) < 6)
            loc[..., 0] = np.where(pl & (where != 1), v, loc[..., 0])
            loc[..., 1] = np.where(pl & (where != 0), v, loc[..., 1])
        elif kind == "all_out":
            if whole:
                pl[:] = True
            else:
                pl[:, int(qs[0]), int(rng.integers(0, M))] = True              # (a) one query and head
                if run is not None:
                    pl[:, run:run + 128] = True
                pl[:, :, :, level::L] = True                                   # (b) one level, in every window slot
                if frame is not None:                                          # (c) one source frame (of every clip)
                    T = d["ftab"].shape[0]
                    for b in range(B):
                        if lk == "loc_c":
                            pl[b] |= (b % T == frame)
                        else:
                            for w, f in enumerate(d["ftab"][b % T]):
                                if f == frame:
                                    pl[b, :, :, w * L:(w + 1) * L] = True
            ou = pl.copy()
            how = rng.integers(0, 4, size=pl.shape)                            # one coordinate leaves the map, the other stays as drawn
            loc[..., 0] = np.where(pl & (how < 2), np.where(how == 0, -3.0, 5.0), loc[..., 0])
            loc[..., 1] = np.where(pl & (how >= 2), np.where(how == 2, -3.0, 5.0), loc[..., 1])
        elif kind == "piled":
            n = max(2, nq) if Lq >= 2 else 1
            q0 = int(rng.integers(0, Lq - n + 1))
            pl[:, q0:q0 + n] = True
            i0, j0 = np.floor(rng.random(H.shape) * H), np.floor(rng.random(W.shape) * W)      # one cell / corner per level slot
            fr = 0.1 + 0.8 * rng.random(pl.shape + (2,))
            around = np.zeros(pl.shape + (2,))
            around[:, q0 + n // 2:q0 + n] = rng.integers(0, 2, size=around[:, q0 + n // 2:q0 + n].shape)       # second half: four cells
            cand = np.stack([(j0 + fr[..., 0] - around[..., 0] + 0.5) / W, (i0 + fr[..., 1] - around[..., 1] + 0.5) / H], -1)
            loc = np.where(pl[..., None], cand, loc)
        elif kind == "weights":
            third = max(1, nq // 3)
            zero, neg, triple = qs[:third], qs[third:2 * third], qs[2 * third:]
            pl[:, qs] = True
            zw[:, zero] = True
            aw[:, zero] = 0.0
            aw[:, neg] = -aw[:, neg]
            aw[:, triple] = 3.0 * aw[:, triple]
        if not (kind == "all_out"):
            assert pl.any(axis=(0, 2, 3, 4)).sum() <= max(1, Lq // 3) or Lq < 3, kind
        r[lk], r[ak] = loc.astype(d[lk].dtype), aw.astype(d[ak].dtype)
        masks["placed"][lk], masks["out"][lk], masks["zero_w"][lk] = pl, ou, zw
    if kind == "all_out" and not whole:
        masks["levels"] = [level]
        if frame is not None:
            T = d["ftab"].shape[0]
            masks["frames"] = [b for b in range(d["value"].shape[0]) if b % T == frame]
    return r, masks


def out_moved(d, masks, to=-10.0):
    """`d` with every location that `masks` marks as out of range replaced by (`to`, `to`): no output may change by a bit."""
    r = dict(d)
    for lk, m in masks["out"].items():
        r[lk] = np.where(m[..., None], np.asarray(to, d[lk].dtype), d[lk])
    return r

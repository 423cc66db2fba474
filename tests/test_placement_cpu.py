"""helpers.place and the oracle alone, without a GPU: on every pyramid tests/test_placement_gpu.py uses, each kind places what
it promises, and the inputs it makes are ones the reference arithmetic has one answer for -- the oracle in fp32 and in fp64 is
finite and warning-free, the two agree on the forward (no disagreement on a range decision), and grad_loc / grad_attn are exactly
0 at every point the masks call out of range.  These are conditions on the inputs; a kind that misses one gets other inputs."""
import warnings

import numpy as np
import pytest
import torch

from helpers import (HUGE, PLACEMENTS, POW2, POW2_4, PYR_A, make_inputs, make_temporal_inputs, oracle_fwd_bwd, out_moved, place,
                     round_to, temporal_reference)

SMALL = [(9, 11), (6, 10), (4, 5), (2, 3)]                 # tests/test_layout_gpu.py
PYR_S = [(20, 33), (10, 17), (5, 9), (3, 5)]               # tests/test_window_gpu.py
TKEYS = ("value", "shapes", "lsi", "ftab", "loc_c", "aw_c", "loc_t", "aw_t", "grad_out")
KINDS = PLACEMENTS + ("all_out_call",)


def _place(d, kind, seed):
    return place(d, "all_out", seed, whole=True) if kind == "all_out_call" else place(d, kind, seed)


def _pyramids(kind):
    return (POW2, POW2_4) if kind in ("on_grid", "edges") else (SMALL, PYR_A, PYR_S)


def _plain(shapes, Lq=37):
    return make_inputs(3, 2, 5, 8, Lq, shapes, 4, "wide", np.float64, value_scale=1.0)


def _temporal(shapes, Lq=60, ftab=None, T=4, W=3):
    return make_temporal_inputs(5, T, W, 3, 8, Lq, shapes, 4, 2, ftab=ftab, dtype=np.float64)


def _in_range(loc, shapes):
    """The reference's range test on [..., LL, P, 2] locations in fp64 (NaN: False)."""
    L = len(shapes)
    H = np.tile(np.asarray(shapes)[:, 0], loc.shape[-3] // L).astype(np.float64)[:, None]
    W = np.tile(np.asarray(shapes)[:, 1], loc.shape[-3] // L).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        h, w = loc[..., 1] * H - 0.5, loc[..., 0] * W - 0.5
        return (h > -1) & (w > -1) & (h < H) & (w < W)


@pytest.mark.parametrize("kind", KINDS)
def test_counts_are_what_the_kind_promises(kind):
    for shapes in _pyramids(kind):
        for Lq in (37, 900):
            d = _plain(shapes, Lq)
            r, m = _place(d, kind, 11)
            pl, ou, zw = m["placed"]["loc"], m["out"]["loc"], m["zero_w"]["loc"]
            B, _, M, L, P = pl.shape
            touched = int(pl.any(axis=(0, 2, 3, 4)).sum())
            same = (r["loc"] == d["loc"]).all(-1) | (np.isnan(r["loc"]) & np.isnan(d["loc"])).all(-1)
            assert same[~pl].all() and (r["aw"] == d["aw"])[~pl].all()          # nothing but the placed points changed
            assert not (ou & ~pl).any() and not _in_range(r["loc"], shapes)[ou].any()
            if kind not in ("all_out", "all_out_call"):
                assert 1 <= touched <= Lq // 3
            if kind in ("on_grid", "edges"):
                assert touched == Lq // 3 and pl.sum() == B * touched * M * L * P
                px = r["loc"] * np.array([s[::-1] for s in shapes], np.float64)[:, None, :] - 0.5
                whole = (px == np.round(px)).any(-1)
                assert whole[pl].all() or kind == "edges"                      # on_grid: a whole pixel coordinate in every point
                if kind == "edges":                                               # per level: all 24 combinations of the two axes
                    for l, (H, W) in enumerate(shapes):
                        y, x = px[:, :, :, l, :, 1][pl[:, :, :, l]], px[:, :, :, l, :, 0][pl[:, :, :, l]]
                        cls = lambda v, n: np.select([v == -1, v == n, v < 0, v > n - 1], [2, 3, 0, 1], 4)      # noqa: E731
                        assert len(set(zip(cls(y, H).tolist(), cls(x, W).tolist()))) == 24 if H > 1 and W > 1 else True
                    assert ou.sum() == (((px == -1) | (px == np.array([s[::-1] for s in shapes])[:, None, :])).any(-1) & pl).sum()
            elif kind == "nonfinite":
                bad = ~np.isfinite(r["loc"])
                assert (bad.any(-1) == pl).all() and (ou == pl).all()
                for v in (np.nan, np.inf, -np.inf):                               # each value in x only, in y only, in both
                    is_v = np.isnan(r["loc"]) if v != v else r["loc"] == v
                    assert (is_v[..., 0] & ~bad[..., 1]).any() and (is_v[..., 1] & ~bad[..., 0]).any() and is_v.all(-1).any()
                whole_rows = pl.all(axis=(2, 3, 4)).any(0)
                whole_groups = pl.all(-1) & ~pl.all(axis=(2, 3, 4))[:, :, None, None]
                part_groups = pl.any(-1) & ~pl.all(-1)
                assert whole_rows.any() and whole_groups.any() and part_groups.any()
                if Lq >= 768:
                    assert any(whole_rows[b:b + 64].all() for b in range(0, Lq - 63, 64))
            elif kind == "huge":
                for v in HUGE:
                    assert ((r["loc"] == v) & (np.signbit(r["loc"]) == np.signbit(v)) & pl[..., None]).any(), v
                assert ou.sum() > 0 and (pl & ~ou).sum() > 0
            elif kind == "all_out":
                l = m["levels"][0]
                assert pl[:, :, :, l].all() and pl.all(axis=(3, 4)).any() and not pl.all()
                if Lq >= 768:
                    assert any(pl[:, b:b + 64].all() for b in range(0, Lq - 63, 64))
            elif kind == "all_out_call":
                assert pl.all() and ou.all() and m["call"]
            elif kind == "piled":
                qs = np.nonzero(pl.any(axis=(0, 2, 3, 4)))[0]
                assert len(qs) >= 2 and (np.diff(qs) == 1).all() and pl[:, qs].all()
                cell = np.floor(r["loc"] * np.array([s[::-1] for s in shapes], np.float64)[:, None, :] - 0.5)
                a, b = cell[:, qs[:len(qs) // 2]], cell[:, qs[len(qs) // 2:]]
                assert (a == a[:1, :1, :1, :, :1]).all()                          # one cell per level
                assert ((b - a[:1, :1, :1, :, :1] >= -1) & (b - a[:1, :1, :1, :, :1] <= 0)).all()
                assert (b != a[:1, :1, :1, :, :1]).any()
            elif kind == "weights":
                s = r["aw"].sum(axis=(-1, -2))
                assert (r["aw"][zw] == 0).all() and zw.any() and (zw.all(axis=(0, 2, 3, 4)) == zw.any(axis=(0, 2, 3, 4))).all()
                assert (s < -0.99).any() and (np.abs(s - 3) < 1e-9).any() and np.isfinite(r["aw"]).all()


def _oracles(r, temporal):
    """(fp32, fp64) oracle outputs, every numpy warning an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            if not temporal:
                return oracle_fwd_bwd(r, np.float32), oracle_fwd_bwd(r, np.float64)
            return tuple(temporal_reference(*(np.asarray(r[k], t) if r[k].dtype.kind == "f" else r[k] for k in TKEYS))
                         for t in (np.float32, np.float64))


def _check_oracle(r, m, temporal):
    r = round_to(r, torch.float32)                       # as the GPU tests do: the oracle sees what the storage type holds
    r32, r64 = _oracles(r, temporal)
    for x in r32 + r64:
        assert np.isfinite(x).all()
    assert np.abs(r32[0] - r64[0]).max() <= 1e-5 * max(1.0, float(np.abs(r64[0]).max()))
    outs = (("loc", 2, 3),) if not temporal else (("loc_c", 2, 3), ("loc_t", 4, 5))
    for res in (r32, r64):
        for lk, gl, ga in outs:
            assert (res[gl][m["out"][lk]] == 0).all() and (res[ga][m["out"][lk]] == 0).all()
            assert (res[gl][m["zero_w"][lk]] == 0).all()
        for l in m["levels"]:
            H, W = r["shapes"][l]
            assert (res[1][:, r["lsi"][l]:r["lsi"][l] + H * W] == 0).all()
        assert (res[1][m["frames"]] == 0).all() if m["frames"] else True
        if m["call"]:
            assert (res[0] == 0).all() and (res[1] == 0).all()
    moved = _oracles(out_moved(r, m), temporal)[1]                               # the metamorphic check holds for the oracle
    assert all(np.array_equal(a, b) for a, b in zip(moved, r64))


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_is_finite_and_agrees_with_itself_on_plain_calls(kind):
    for shapes in _pyramids(kind):
        r, m = _place(_plain(shapes, 900 if shapes is PYR_S else 37), kind, 13)
        _check_oracle(r, m, False)
    if kind not in ("on_grid", "edges"):
        r, m = _place(_plain([(2, 1100), (3, 5)], 23), kind, 14)                  # the level wider than a band
        _check_oracle(r, m, False)


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_is_finite_and_agrees_with_itself_on_temporal_calls(kind):
    rep = np.array([[1, 1], [0, 2], [1, 3], [2, 4], [3, 3]], dtype=np.int32)     # repeated and missing frames
    for shapes in _pyramids(kind)[:2]:
        r, m = _place(_temporal(shapes), kind, 17)
        _check_oracle(r, m, True)
        r, m = _place(_temporal(shapes, ftab=rep, T=5, W=2), kind, 19)
        _check_oracle(r, m, True)
        if kind == "all_out":
            assert m["frames"] and len(m["levels"]) == 1


def test_rounding_to_16_bits_keeps_the_exact_kinds_and_the_masks():
    """on_grid / edges coordinates are unchanged by bf16 / f16 storage; the huge values stay out of range in every type."""
    for kind in ("on_grid", "edges"):
        r, m = place(_plain(POW2), kind, 23)
        for t in (torch.bfloat16, torch.float16):
            q = round_to({"loc": r["loc"]}, t)["loc"]
            assert np.array_equal(q[m["placed"]["loc"]], r["loc"][m["placed"]["loc"]])
    r, m = place(_plain(SMALL), "huge", 29)
    for t in (torch.float32, torch.bfloat16, torch.float16):
        q = round_to({"loc": r["loc"]}, t)["loc"]
        assert not _in_range(q, SMALL)[m["out"]["loc"]].any()

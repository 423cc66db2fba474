"""Backward time of the full, GRAD_VALUE-only and GRAD_SAMPLING-only calls (msda_backward_grads / msda_temporal_backward_grads),
timed in interleaved blocks -- full, value, sampling, full, ... -- with device events after a warm-up; one JSON line per case
with the median ms of each mode.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` (a run of its own).
    python scripts/grad_subset_bench.py [--blocks 8] [--iters 10]
Cases: cfg3 (16 clips, T=6, 300 queries, pyramid 360x640) in fp32 and bf16, the one-clip decoder call DeVIS issues, the one-clip
temporal encoder at 360x640 (Lq = S, local sampling), and BASELINE configs[1] (single-frame encoder attention, 800x1333, N=8, bf16)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from devis_amd import _native  # noqa: E402

PYR_A = [(45, 80), (23, 40), (12, 20), (6, 10)]
PYR_B = [(100, 167), (50, 84), (25, 42), (13, 21)]
M, D, P = 8, 32, 4
VALUE, SAMPLING, ALL = _native.GRAD_VALUE, _native.GRAD_SAMPLING, _native.GRAD_ALL


def _locs(g, N, Lq, L, shapes, local):
    if not local:
        return torch.rand(N, Lq, M, L, P, 2, generator=g)
    sh = torch.tensor(shapes, dtype=torch.float32)
    centres = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij"),
                                     -1).reshape(-1, 2).flip(-1) for h, w in shapes], 0)
    wh = torch.stack([sh[:, 1], sh[:, 0]], -1)
    Lw = L // len(shapes)
    return centres[None, :, None, None, None, :] + torch.randn(N, Lq, M, L, P, 2, generator=g) * 2.0 / wh.repeat(Lw, 1)[None, None, None, :, None, :]


def temporal_case(clips, T, Lq, shapes, dtype, local=False):
    g = torch.Generator().manual_seed(0)
    G, L, W = clips * T, len(shapes), T - 1
    sh = torch.tensor(shapes, dtype=torch.int64)
    S = int(sh.prod(1).sum())
    Lq = S if Lq is None else Lq
    d = lambda x: x.to("cuda", dtype).contiguous()          # noqa: E731
    t = dict(value=d(torch.rand(G, S, M, D, generator=g) * 2 - 1), shapes=sh.cuda(),
             lsi=torch.cat((sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1])).cuda(),
             ftab=torch.tensor([[f for f in range(T) if f != t] for t in range(T)], dtype=torch.int32, device="cuda"),
             loc_c=d(_locs(g, G, Lq, L, shapes, local)), loc_t=d(_locs(g, G, Lq, W * L, shapes, local)),
             grad_out=d(torch.randn(G, Lq, M * D, generator=g)))
    aw = torch.softmax(torch.randn(G, Lq, M, (L + W * L) * P, generator=g), -1)
    t["aw_c"], t["aw_t"] = d(aw[..., :L * P].reshape(G, Lq, M, L, P)), d(aw[..., L * P:].reshape(G, Lq, M, W * L, P))
    gv = torch.empty(t["value"].shape, dtype=_native.grad_value_dtype(t["value"], t["shapes"], Lq, L, P, clips=clips, window=W, Pt=P),
                     device="cuda")
    gs = [torch.empty_like(t[k]) for k in ("loc_c", "aw_c", "loc_t", "aw_t")]
    ws = _native.bwd_workspace(t["value"].device, G, Lq, M, L * (1 + W))
    args = (t["value"], t["shapes"], t["lsi"], t["ftab"], t["loc_c"], t["aw_c"], t["loc_t"], t["aw_t"], t["grad_out"], clips)

    def run(grads):
        if grads == ALL:
            _native.temporal_backward(*args, gv, *gs, workspace=ws)
        else:
            _native.temporal_backward_grads(grads, *args, gv if grads & VALUE else None,
                                            *(gs if grads & SAMPLING else [None] * 4), workspace=ws if grads & VALUE else None)
    return run


def plain_case(N, shapes, dtype):
    """Single-frame encoder attention: Lq = S, local sampling."""
    g = torch.Generator().manual_seed(1)
    sh = torch.tensor(shapes, dtype=torch.int64)
    L, S = len(shapes), int(sh.prod(1).sum())
    d = lambda x: x.to("cuda", dtype).contiguous()          # noqa: E731
    value, loc = d(torch.rand(N, S, M, D, generator=g) * 2 - 1), d(_locs(g, N, S, L, shapes, True))
    aw = d(torch.softmax(torch.randn(N, S, M, L * P, generator=g), -1).reshape(N, S, M, L, P))
    go = d(torch.randn(N, S, M * D, generator=g))
    shapes_d, lsi = sh.cuda(), torch.cat((sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1])).cuda()
    gv = torch.empty(value.shape, dtype=_native.grad_value_dtype(value, shapes_d, S, L, P), device="cuda")
    gl, ga = torch.empty_like(loc), torch.empty_like(aw)
    ws = _native.bwd_workspace(value.device, N, S, M, L)

    def run(grads):
        if grads == ALL:
            _native.backward(value, shapes_d, lsi, loc, aw, go, gv, gl, ga)
        else:
            _native.backward_grads(grads, value, shapes_d, lsi, loc, aw, go, gv if grads & VALUE else None,
                                   gl if grads & SAMPLING else None, ga if grads & SAMPLING else None,
                                   workspace=ws if grads & VALUE else None)
    return run


def measure(run, blocks, iters):
    modes = {"full": ALL, "value": VALUE, "sampling": SAMPLING}
    for g in modes.values():                    # warm-up (LDS opt-ins, caches)
        for _ in range(3):
            run(g)
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    routes = {}
    for _ in range(blocks):
        for name, g in modes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                run(g)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / iters)
            routes[name] = _native.last_route()
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    _native.load()
    cases = [
        ("cfg3_16clips_f32", lambda: temporal_case(16, 6, 300, PYR_A, torch.float32)),
        ("cfg3_16clips_bf16", lambda: temporal_case(16, 6, 300, PYR_A, torch.bfloat16)),
        ("decoder_1clip_f32", lambda: temporal_case(1, 6, 300, PYR_A, torch.float32)),
        ("temporal_encoder_1clip_360x640_f32", lambda: temporal_case(1, 6, None, PYR_A, torch.float32, local=True)),
        ("baseline_cfg1_encoder_800x1333_bf16", lambda: plain_case(8, PYR_B, torch.bfloat16)),
    ]
    for name, make in cases:
        ms, routes = measure(make(), args.blocks, args.iters)
        print(json.dumps({"case": name, "ms": ms, "value_vs_full": round(ms["value"] / ms["full"], 3),
                          "sampling_vs_full": round(ms["sampling"] / ms["full"], 3), "routes": routes}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

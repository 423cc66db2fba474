"""Times devis_amd.attention_maps on the three pyramid levels of a 360x640 clip (12x20, 23x40, 45x80) and of an 800x1333 one
(25x42, 50x84, 100x167): B = 6, Q in {10, 50}, n = 8, c = 32, padding masks; f32, and bf16 with float32 maps; forward and
forward + backward.  The baseline is the PyTorch formulation of the oracle (einsum, masked_fill, softmax) on the same GPU, in
the same process and dtype (for bf16: softmax to float32, what autocast runs).

    python scripts/attmap_bench.py [--out profiles/attmap_bench.json] [--windows 5] [--iters 200]

Device events after warm-up; operator and baseline windows alternate; the median of the windows is quoted, and "spread" is
(max - min) / median over them.  "hbm_fraction" is the algorithmic bytes of the fused operator -- out written once, plus q, k
and mask read in each of the two passes; backward: out and grad_out read in each of its two passes, dl written, then dl, q and
k read and a gradient written by each GEMM -- over the operator's time, as a fraction of 8 TB/s.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAPS = [("360x640", 12, 20), ("360x640", 23, 40), ("360x640", 45, 80), ("800x1333", 25, 42), ("800x1333", 50, 84),
        ("800x1333", 100, 167)]
B, HEADS, C = 6, 8, 32
QUERIES = (10, 50)
HBM_BYTES_PER_S = 8e12


def make(Q, H, W, dtype, out_dtype, dev):
    gen = torch.Generator().manual_seed(Q * H + W)
    q = torch.randn(B, Q, HEADS * C, generator=gen).to(dev, dtype)
    k = torch.randn(B, HEADS * C, H, W, generator=gen).to(dev, dtype)
    mask = torch.zeros(B, H, W, dtype=torch.bool)
    for b in range(B):      # padding: image b keeps a little less of the right and bottom edges
        mask[b, :, W - (b * W) // 24:] = b > 0
        mask[b, H - (b * H) // 32:, :] = b > 0
    g = torch.randn(B, Q, HEADS, H, W, generator=gen).to(dev, out_dtype)
    return q, k, mask.to(dev), g


def baseline(q, k, mask, out_dtype):
    Bq, Q, D = q.shape
    H, W = k.shape[-2:]
    w = torch.einsum("bqnc,bnchw->bqnhw", q.view(Bq, Q, HEADS, C) * C ** -0.5, k.view(Bq, HEADS, C, H, W))
    w = w.masked_fill(mask[:, None, None], float("-inf"))
    return torch.softmax(w.flatten(2), dim=-1, dtype=out_dtype).view_as(w)


def algorithmic_bytes(Q, H, W, dtype, out_dtype, backward):
    es, eo, P = torch.empty((), dtype=dtype).element_size(), torch.empty((), dtype=out_dtype).element_size(), H * W
    nq, nk, nout = B * Q * HEADS * C, B * HEADS * C * P, B * Q * HEADS * P
    fwd = nout * eo + 2 * (nq * es + nk * es + B * P)
    if not backward:
        return fwd
    return fwd + 2 * 2 * nout * eo + nout * es + 2 * (nout * es + nq * es + nk * es) + (nq + nk) * es


def stepper(fn, q, k, g, backward):
    if not backward:
        def step():
            with torch.no_grad():
                fn(q, k)
        return step
    leaves = [t.detach().requires_grad_(True) for t in (q, k)]

    def step():
        torch.autograd.grad(fn(*leaves), leaves, g)
    return step


def window(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attmap_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)      # windows of 5-120 ms: shorter ones time the host's jitter
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attmap_bench needs the GPU: there is no CPU path to time")
    import devis_amd
    dev = torch.device("cuda:0")
    rows = []
    for dtype, out_dtype, label in ((torch.float32, torch.float32, "f32"), (torch.bfloat16, torch.float32, "bf16->f32")):
        for clip, H, W in MAPS:
            for Q in QUERIES:
                q, k, mask, g = make(Q, H, W, dtype, out_dtype, dev)
                ours = lambda q, k: devis_amd.attention_maps(q, k, mask, num_heads=HEADS, out_dtype=out_dtype)    # noqa: E731
                theirs = lambda q, k: baseline(q, k, mask, out_dtype)       # noqa: E731
                for backward in (False, True):
                    steps = [stepper(fn, q, k, g, backward) for fn in (ours, theirs)]
                    for s in steps:
                        for _ in range(3):
                            s()
                    torch.cuda.synchronize()
                    times = ([], [])
                    for _ in range(args.windows):       # alternating windows
                        for t, s in zip(times, steps):
                            t.append(window(s, args.iters))
                    med = [statistics.median(t) for t in times]
                    spread = [(max(t) - min(t)) / m for t, m in zip(times, med)]
                    nbytes = algorithmic_bytes(Q, H, W, dtype, out_dtype, backward)
                    row = {"clip": clip, "H": H, "W": W, "B": B, "Q": Q, "heads": HEADS, "c": C, "dtype": label,
                           "pass": "fwd+bwd" if backward else "fwd", "operator_us": round(med[0], 2),
                           "baseline_us": round(med[1], 2), "operator_spread": round(spread[0], 4),
                           "baseline_spread": round(spread[1], 4), "speedup": round(med[1] / med[0], 3),
                           "faster_by_more_than_the_spread": bool(max(times[0]) < min(times[1])),
                           "algorithmic_bytes": nbytes, "hbm_fraction": round(nbytes / (med[0] * 1e-6) / HBM_BYTES_PER_S, 4),
                           "operator_windows_us": [round(v, 2) for v in times[0]],
                           "baseline_windows_us": [round(v, 2) for v in times[1]]}
                    rows.append(row)
                    print(json.dumps({k_: row[k_] for k_ in ("dtype", "H", "W", "Q", "pass", "operator_us", "baseline_us",
                                                              "speedup", "hbm_fraction", "faster_by_more_than_the_spread")}),
                          flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "iters": args.iters,
           "method": "device events; median of alternating windows; spread = (max - min) / median", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

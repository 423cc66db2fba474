"""Times the matchers' assignment on devis_amd.linear_assignment (patch_criterion(gpu_assignment=True)) against the path it
replaces -- the cost's device-to-host transfer, scipy.optimize.linear_sum_assignment on the host, the index tensors copied
back -- on the same GPU, in the same process, on the same inputs.

    solver      the assignment alone, from a cost [L, R, T] on the device to index tensors on the device, for L in {1, 6} and
                R x T in {50 x 1, 50 x 5, 50 x 10, 50 x 25, 300 x 25, 100 x 100}; random costs, and the rank-one worst case
                -outer(a, b) of sorted factors, on which the method takes its n(n+1)/2 dependent steps.
    matcher     one patched DeVISHungarianMatcher call at F = 6, Q = 50, C = 40 and T in {1, 5, 10, 25} targets, and the six
                decoder layers of a criterion call through batch_aux: the host path against gpu_assignment.

Beside the times, per call: the synchronising calls torch.cuda.set_sync_debug_mode("warn") reports.  Both sides must return
the same indices.

    python scripts/assign_bench.py [--out profiles/assign_bench.json] [--windows 7] [--iters 20]

Method: every side is warmed up; a window is `iters` calls between a device synchronise and a host clock read after another
one; the windows of the sides alternate; the median of the windows is quoted and every window is kept.  The device side does
not wait for its results inside a window: its time is the cost of a call to a host that keeps enqueueing, which is how a
training step uses it; "latency_ms" is one call followed by a synchronise.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types
import warnings

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, QUERIES, CLASSES = 6, 50, 40
TARGETS = (1, 5, 10, 25)
LAYERS = 6
PROBLEMS = (1, 6)
SHAPES = ((50, 1), (50, 5), (50, 10), (50, 25), (300, 25), (100, 100))


class Matcher(torch.nn.Module):
    """The attributes patch_criterion reads of a DeVISHungarianMatcher; its own forward is never reached."""
    cost_class, cost_bbox, cost_giou, focal_loss, focal_alpha = 2.0, 5.0, 2.0, True, 0.25
    num_frames, num_out, use_l1_distance_sum = FRAMES, QUERIES, False

    def forward(self, outputs, targets):
        raise NotImplementedError


class Criterion:
    """Enough of a criterion for patch_criterion(batch_aux=True): ``forward`` returns the matchings, top level first."""

    def __init__(self, matcher):
        self.matcher = matcher

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        raise NotImplementedError

    def forward(self, outputs, targets):
        return [d["indices"] if "indices" in d else self.matcher({k: v for k, v in d.items() if k != "aux_outputs"}, targets)
                for d in (outputs, *outputs.get("aux_outputs", ()))]


def patched_pair(devis_amd, **keywords):
    """(matcher, criterion) of fresh stand-in classes under patch_criterion(batch_aux=True, **keywords)."""
    crit = types.SimpleNamespace(SetCriterion=type("SetCriterion", (Criterion,), {}))
    match = types.SimpleNamespace(DeVISHungarianMatcher=type("DeVISHungarianMatcher", (Matcher,), {}),
                                  HungarianMatcher=type("HungarianMatcher", (torch.nn.Module,), {}))
    devis_amd.patch_criterion(crit, match, batch_aux=True, **keywords)
    matcher = match.DeVISHungarianMatcher()
    return matcher, crit.SetCriterion(matcher)


def host_assignment(cost):
    """The replaced path on a device cost [L, R, T]: one transfer, scipy per problem, the indices back without a second
    synchronisation."""
    pairs = [linear_sum_assignment(c) for c in cost.cpu().numpy()]
    rows = torch.as_tensor(np.stack([p[0] for p in pairs]), dtype=torch.int64).pin_memory().to(cost.device, non_blocking=True)
    cols = torch.as_tensor(np.stack([p[1] for p in pairs]), dtype=torch.int64).pin_memory().to(cost.device, non_blocking=True)
    return rows, cols


def rank_one(n, m, rng):
    a, b = np.sort(rng.rand(n).astype(np.float32)), np.sort(rng.rand(m).astype(np.float32))
    return -np.outer(a, b).astype(np.float32)


def boxes_of(g, *shape):
    return torch.cat([0.2 + 0.6 * torch.rand(*shape, 2, generator=g), 0.05 + 0.45 * torch.rand(*shape, 2, generator=g)], -1)


def window(fn, iters):
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3 / iters


def syncs_of(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("called a synchronizing" in str(w.message) for w in seen)


def compare(sides, windows, iters):
    """{name: fn} -> {name: {"ms": median, "windows_ms": [...], "latency_ms", "synchronisations"}}, the windows alternating."""
    for fn in sides.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            times[k].append(window(fn, iters))
    return {k: {"ms": statistics.median(times[k]), "windows_ms": times[k],
                "latency_ms": statistics.median(window(fn, 1) for _ in range(windows)), "synchronisations": syncs_of(fn)}
            for k, fn in sides.items()}


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("assign_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    dev = torch.device("cuda:0")
    rng, g = np.random.RandomState(0), torch.Generator().manual_seed(0)

    solver_rows = []
    for R, T in SHAPES:
        for L in PROBLEMS:
            for kind in ("random", "rank_one"):
                host = np.stack([rng.standard_normal((R, T)).astype(np.float32) if kind == "random" else rank_one(R, T, rng)
                                 for _ in range(L)])
                cost = torch.from_numpy(host).to(dev)
                rows, cols, status = devis_amd.linear_assignment(cost)
                equal = same(host_assignment(cost), (rows, cols)) and status.tolist() == [0, 0]
                res = compare({"host": lambda: host_assignment(cost), "device": lambda: devis_amd.linear_assignment(cost)},      # noqa: B023
                              args.windows, args.iters)
                solver_rows.append({"rows": R, "cols": T, "problems": L, "costs": kind, "same_indices": equal,
                                    "host_over_device": res["host"]["ms"] / res["device"]["ms"], **res})
                print("%3d x %3d, L = %d, %-8s: host %.3f ms (latency %.3f), device %.3f ms (latency %.3f)%s"
                      % (R, T, L, kind, res["host"]["ms"], res["host"]["latency_ms"], res["device"]["ms"],
                         res["device"]["latency_ms"], "" if equal else "  INDICES DIFFER"), flush=True)

    (host_matcher, host_criterion), (gpu_matcher, gpu_criterion) = patched_pair(devis_amd), patched_pair(devis_amd, gpu_assignment=True)

    def layer():
        return {"pred_logits": (2 * torch.randn(1, FRAMES * QUERIES, CLASSES, generator=g)).to(dev),
                "pred_boxes": boxes_of(g, 1, FRAMES * QUERIES).to(dev)}

    matcher_rows = []
    for T in TARGETS:
        targets = [{"labels": torch.randint(0, CLASSES, (T * FRAMES,), generator=g).to(dev), "boxes": boxes_of(g, T * FRAMES).to(dev),
                    "valid": (torch.rand(T * FRAMES, generator=g) > 0.2).to(dev)}]
        layers = [layer() for _ in range(LAYERS)]
        outputs = dict(layers[0], aux_outputs=layers[1:])
        equal = same(host_matcher(layers[0], targets)[0], gpu_matcher(layers[0], targets)[0]) and all(
            same(a[0], b[0]) for a, b in zip(host_criterion.forward(outputs, targets), gpu_criterion.forward(outputs, targets)))
        one = compare({"host": lambda: host_matcher(layers[0], targets), "device": lambda: gpu_matcher(layers[0], targets)},      # noqa: B023
                      args.windows, args.iters)
        six = compare({"host": lambda: host_criterion.forward(outputs, targets), "device": lambda: gpu_criterion.forward(outputs, targets)},      # noqa: B023
                      args.windows, args.iters)
        matcher_rows.append({"targets": T, "same_indices": equal,
                             "matcher": dict(one, host_over_device=one["host"]["ms"] / one["device"]["ms"]),
                             "batch_aux_six_layers": dict(six, host_over_device=six["host"]["ms"] / six["device"]["ms"])})
        print("T = %2d: matcher host %.3f ms, device %.3f ms; six layers through batch_aux host %.3f ms, device %.3f ms; "
              "synchronisations %d and %d against %d and %d%s"
              % (T, one["host"]["ms"], one["device"]["ms"], six["host"]["ms"], six["device"]["ms"], one["host"]["synchronisations"],
                 six["host"]["synchronisations"], one["device"]["synchronisations"], six["device"]["synchronisations"],
                 "" if equal else "  INDICES DIFFER"), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "shape": {"frames": FRAMES, "queries": QUERIES, "classes": CLASSES, "layers": LAYERS},
           "method": "a window is `iters` calls between device synchronises, by a host clock; windows of the sides alternate; "
                     "medians quoted; latency_ms is the median of windows of one call; synchronisations are per call, by "
                     "torch.cuda.set_sync_debug_mode; host = transfer, scipy, indices copied back (the path gpu_assignment replaces)",
           "solver": solver_rows, "matcher": matcher_rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Times the criterion's matching and box losses on devis_amd.match_cost / devis_amd.box_losses (patch_criterion) against the
formulation they replace, on the same GPU, in the same process.

    matcher     one DeVISHungarianMatcher call at F = 6, Q = 50, C = 40 and T in {1, 5, 10} targets, from the decoder outputs to
                the index tensors: cost, host copy and scipy's assignment included.
    layers      the matchings of six decoder layers: six patched calls against one batch_aux call (one cost launch, one
                transfer, six assignments), and against six calls of the replaced formulation.
    loss_boxes  forward and backward of the two box losses at N in {6, 60} matched boxes.

The replaced side is a restatement, in this script, of what the stock matcher and loss compute with torch operators (the
[Q, T, F, 4] temporaries, the class cost on every logit, the degenerate-box checks that synchronise, the Python loop over the
matches; the N x N GIoU matrix whose diagonal is the loss).  Both sides get the same tensors and must return the same indices.

Beside the times, per call: the ATen operators dispatched (torch's dispatch mode), the kernel launches of this library, the
device activities a torch.profiler trace lists (kernels, copies, memsets; "not measured" where the profiler gives none), and
the synchronising calls torch.cuda.set_sync_debug_mode("warn") reports.

    python scripts/boxmatch_bench.py [--out profiles/boxmatch_bench.json] [--windows 7] [--iters 20]

Method: every side is warmed up; a window is `iters` calls between a device synchronise and a host clock read after another
one; the windows of the sides alternate; the median of the windows is quoted and every window is kept.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types
import warnings

import torch
from scipy.optimize import linear_sum_assignment
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, QUERIES, CLASSES = 6, 50, 40
TARGETS = (1, 5, 10)
LAYERS = 6
PAIRS = (6, 60)
WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)


# ---- the replaced formulation, restated -------------------------------------------------------------------------------------

def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def stock_giou(a, b):
    """GIoU of broadcastable xyxy boxes with the two checks that read the device."""
    assert (a[..., 2:] >= a[..., :2]).all()
    assert (b[..., 2:] >= b[..., :2]).all()
    lo, hi = torch.max(a[..., :2], b[..., :2]), torch.min(a[..., 2:], b[..., 2:])
    wh = (hi - lo).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    size_a, size_b = a[..., 2:] - a[..., :2], b[..., 2:] - b[..., :2]
    union = size_a[..., 0] * size_a[..., 1] + size_b[..., 0] * size_b[..., 1] - inter
    iou = (inter + 1e-6) / (union + 1e-6)
    hull = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    area = hull[..., 0] * hull[..., 1]
    return iou - ((area - union) + 1e-6) / (area + 1e-6)


class StockMatcher(torch.nn.Module):
    """The attributes patch_criterion's matcher reads, and the stock computation as ``forward``."""

    def __init__(self, alpha=0.25):
        super().__init__()
        self.cost_class, self.cost_bbox, self.cost_giou = WEIGHTS["cost_class"], WEIGHTS["cost_bbox"], WEIGHTS["cost_giou"]
        self.num_frames, self.num_out, self.focal_loss, self.focal_alpha, self.use_l1_distance_sum = FRAMES, QUERIES, True, alpha, False

    @torch.no_grad()
    def forward(self, outputs, targets):
        F, Q = self.num_frames, self.num_out
        prob, boxes = outputs["pred_logits"][0].sigmoid(), outputs["pred_boxes"][0]
        labels, tgt, valid = targets[0]["labels"], targets[0]["boxes"], targets[0]["valid"]
        T = len(labels) // F
        neg = (1 - self.focal_alpha) * prob ** 2.0 * (-(1 - prob + 1e-8).log())
        pos = self.focal_alpha * (1 - prob) ** 2.0 * (-(prob + 1e-8).log())
        per_class = (pos.reshape(F, Q, -1).permute(1, 0, 2) - neg.reshape(F, Q, -1).permute(1, 0, 2))
        frame = torch.arange(F).repeat(T)
        cls = per_class[:, frame, labels].view(Q, T, F).mean(-1)
        b = boxes.reshape(F, Q, 4).permute(1, 0, 2).unsqueeze(1)
        g = tgt.reshape(T, F, 4).unsqueeze(0)
        l1 = (b - g).abs().mean((-1, -2))
        giou = -stock_giou(xyxy(b), xyxy(g)).mean(-1)
        cost = self.cost_class * cls + self.cost_bbox * l1 + self.cost_giou * giou
        rows, cols = linear_sum_assignment(cost.cpu())
        valid = valid.reshape(T, F)
        index_i, index_j, index_valid = [], [], []
        for r, c in zip(rows, cols):
            frames = torch.arange(F)
            index_i.append(frames * Q + r)
            index_j.append(frames + c * F)
            index_valid.append(valid[c].type(torch.bool))
        return [(torch.cat(index_i).long(), torch.cat(index_j).long(), torch.cat(index_valid))]


def stock_loss_boxes(src, target, num_boxes):
    a, b = xyxy(src), xyxy(target)
    giou = stock_giou(a[:, None], b[None])                # N x N, for its diagonal
    l1 = torch.nn.functional.l1_loss(src, target, reduction="none")
    return {"loss_bbox": l1.sum() / num_boxes, "loss_giou": (1 - torch.diag(giou)).sum() / num_boxes}


class Criterion:
    """Enough of a criterion for patch_criterion(batch_aux=True): ``forward`` returns the matchings, top level first."""

    def __init__(self, matcher):
        self.matcher = matcher

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        raise NotImplementedError

    def forward(self, outputs, targets):
        return [d["indices"] if "indices" in d else self.matcher({k: v for k, v in d.items() if k != "aux_outputs"}, targets)
                for d in (outputs, *outputs.get("aux_outputs", ()))]


# ---- measuring -----------------------------------------------------------------------------------------------------------

def boxes_of(g, *shape):
    return torch.cat([0.2 + 0.6 * torch.rand(*shape, 2, generator=g), 0.05 + 0.45 * torch.rand(*shape, 2, generator=g)], -1)


def window(fn, iters):
    torch.cuda.synchronize()
    start = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3 / iters


class _Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def counts_of(fn):
    """Per call of fn: ATen operators dispatched, this library's kernel launches, device activities of a profiler trace,
    synchronising calls."""
    from devis_amd import _boxmatch
    launches = []
    originals = {name: getattr(_boxmatch, name) for name in ("cost", "loss_forward", "loss_backward")}
    for name, orig in originals.items():
        setattr(_boxmatch, name, lambda *a, _orig=orig, _name=name: launches.append(_name) or _orig(*a))
    try:
        with _Count() as mode:
            fn()
    finally:
        for name, orig in originals.items():
            setattr(_boxmatch, name, orig)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = sum("called a synchronizing" in str(w.message) for w in seen)
    activities = "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        activities = n if n else "not measured"
    except Exception as exc:        # (a profiler that cannot trace here must not stop the timing)
        activities = "not measured: %s" % type(exc).__name__
    return {"aten_calls": mode.n, "library_launches": len(launches), "device_activities": activities, "synchronisations": syncs}


def compare(sides, windows, iters):
    """{name: fn} -> {name: {"ms": median, "windows_ms": [...], counts}}, the sides' windows alternating."""
    for fn in sides.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            times[k].append(window(fn, iters))
    return {k: dict({"ms": statistics.median(times[k]), "windows_ms": times[k]}, **counts_of(fn)) for k, fn in sides.items()}


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxmatch_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boxmatch_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    class Patched(StockMatcher):
        pass

    class Image(torch.nn.Module):
        pass

    crit = types.SimpleNamespace(SetCriterion=type("SetCriterion", (Criterion,), {}))
    match = types.SimpleNamespace(DeVISHungarianMatcher=Patched, HungarianMatcher=Image)
    devis_amd.patch_criterion(crit, match, batch_aux=True)
    stock, patched = StockMatcher(), Patched()
    criterion = crit.SetCriterion(patched)

    def layer():
        return {"pred_logits": (2 * torch.randn(1, FRAMES * QUERIES, CLASSES, generator=g)).to(dev),
                "pred_boxes": boxes_of(g, 1, FRAMES * QUERIES).to(dev)}

    matcher_rows, layer_rows, loss_rows = [], [], []
    for T in TARGETS:
        targets = [{"labels": torch.randint(0, CLASSES, (T * FRAMES,), generator=g).to(dev), "boxes": boxes_of(g, T * FRAMES).to(dev),
                    "valid": (torch.rand(T * FRAMES, generator=g) > 0.2).to(dev)}]
        layers = [layer() for _ in range(LAYERS)]
        outputs = dict(layers[0], aux_outputs=layers[1:])
        equal = same(stock(layers[0], targets)[0], patched(layers[0], targets)[0])
        res = compare({"replaced": lambda: stock(layers[0], targets), "patched": lambda: patched(layers[0], targets)},
                      args.windows, args.iters)
        matcher_rows.append({"targets": T, "same_indices": equal, "replaced_over_patched": res["replaced"]["ms"] / res["patched"]["ms"], **res})
        per_layer = [patched(d, targets) for d in layers]
        equal = all(same(a[0], b[0]) for a, b in zip(criterion.forward(outputs, targets), per_layer))
        res = compare({"replaced_x6": lambda: [stock(d, targets) for d in layers],
                       "patched_x6": lambda: [patched(d, targets) for d in layers],
                       "batch_aux": lambda: criterion.forward(outputs, targets)}, args.windows, args.iters)
        layer_rows.append({"targets": T, "layers": LAYERS, "same_indices": equal,
                           "patched_x6_over_batch_aux": res["patched_x6"]["ms"] / res["batch_aux"]["ms"],
                           "replaced_x6_over_batch_aux": res["replaced_x6"]["ms"] / res["batch_aux"]["ms"], **res})
        print("T = %2d: matcher replaced %.3f ms, patched %.3f ms; six layers replaced %.3f ms, patched %.3f ms, batch_aux %.3f ms"
              % (T, matcher_rows[-1]["replaced"]["ms"], matcher_rows[-1]["patched"]["ms"], res["replaced_x6"]["ms"],
                 res["patched_x6"]["ms"], res["batch_aux"]["ms"]), flush=True)
    for N in PAIRS:
        src, target = boxes_of(g, N).to(dev).requires_grad_(True), boxes_of(g, N).to(dev)

        def run(fn):
            out = fn(src, target, 4.0)
            grad, = torch.autograd.grad(out["loss_bbox"] + out["loss_giou"], src)
            return out, grad

        (a, ga), (b, gb) = run(stock_loss_boxes), run(devis_amd.box_losses)
        diff = max(float((a[k] - b[k]).detach().abs()) for k in a), float((ga - gb).abs().max())
        res = compare({"replaced": lambda: run(stock_loss_boxes), "patched": lambda: run(devis_amd.box_losses)}, args.windows, args.iters)
        loss_rows.append({"pairs": N, "max_loss_difference": diff[0], "max_gradient_difference": diff[1],
                          "replaced_over_patched": res["replaced"]["ms"] / res["patched"]["ms"], **res})
        print("N = %2d: loss_boxes forward + backward replaced %.3f ms, patched %.3f ms" % (N, res["replaced"]["ms"], res["patched"]["ms"]),
              flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "shape": {"frames": FRAMES, "queries": QUERIES, "classes": CLASSES},
           "method": "a window is `iters` calls between device synchronises, by a host clock; windows of the sides alternate; "
                     "medians quoted; counts are per call: ATen operators by torch's dispatch mode, this library's kernel launches, "
                     "device activities of a torch.profiler trace, synchronising calls by torch.cuda.set_sync_debug_mode",
           "matcher": matcher_rows, "layers": layer_rows, "loss_boxes": loss_rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

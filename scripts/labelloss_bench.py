"""Times the criterion's label loss on devis_amd.label_losses (patch_label_loss) against the formulation it replaces, on the
same GPU, in the same process: forward and backward of SetCriterion.loss_labels_focal for one decoder layer at F = 6, Q = 50,
C = 40 and T in {5, 10} targets, from the logits and the matcher's index triple -- on the device, as
patch_criterion(gpu_assignment=True) leaves it -- to d loss_ce / d logits, class_error included.

The replaced side is a restatement, in this script, of what the stock method computes with torch operators (the two
boolean-mask index operations that synchronise, full / index_put / zeros / scatter_ / slice, sigmoid_focal_loss, accuracy's
topk).  Both sides get the same tensors and must return the same loss_ce within 1e-4 * max(1, |loss_ce|).

Beside the times, per call: the ATen operators dispatched (torch's dispatch mode), the kernel launches of this library, the
device activities a torch.profiler trace lists (kernels, copies, memsets; "not measured" where the profiler gives none), and
the synchronising calls torch.cuda.set_sync_debug_mode("warn") reports.

    python scripts/labelloss_bench.py [--out profiles/labelloss_bench.json] [--windows 7] [--iters 20]

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
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, QUERIES, CLASSES = 6, 50, 40
TARGETS = (5, 10)
ALPHA = 0.25


# ---- the replaced formulation, restated -------------------------------------------------------------------------------------

def stock_accuracy(output, target):
    if target.numel() == 0:
        return torch.zeros([], device=output.device)
    _, pred = output.topk(1, 1, True, True)
    correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
    return correct[:1].reshape(-1).float().sum(0).mul_(100.0 / target.size(0))


class StockCriterion:
    """The attributes the drop-in reads, and the stock computation as ``loss_labels_focal``."""
    focal_alpha = ALPHA

    def loss_labels_focal(self, outputs, targets, indices, num_boxes, log=True):
        logits = outputs["pred_logits"]
        C = logits.shape[2]
        batch = torch.cat([torch.full_like(src, i)[mask] for i, (src, _, mask) in enumerate(indices)])
        src = torch.cat([src[mask] for (src, _, mask) in indices])
        wanted = torch.cat([t["labels"][J[mask]] for t, (_, J, mask) in zip(targets, indices)])
        classes = torch.full(logits.shape[:2], C, dtype=torch.int64, device=logits.device)
        classes[(batch, src)] = wanted
        onehot = torch.zeros([logits.shape[0], logits.shape[1], C + 1], dtype=logits.dtype, layout=logits.layout, device=logits.device)
        onehot.scatter_(2, classes.unsqueeze(-1), 1)
        onehot = onehot[:, :, :-1]
        prob = logits.sigmoid()
        ce = torch.nn.functional.binary_cross_entropy_with_logits(logits, onehot, reduction="none")
        p_t = prob * onehot + (1 - prob) * (1 - onehot)
        loss = ce * ((1 - p_t) ** 2)
        loss = (self.focal_alpha * onehot + (1 - self.focal_alpha) * (1 - onehot)) * loss
        losses = {"loss_ce": loss.mean(1).sum() / num_boxes * logits.shape[1]}
        if log:
            losses["class_error"] = 100 - stock_accuracy(logits[(batch, src)], wanted)
        return losses


# ---- measuring -----------------------------------------------------------------------------------------------------------

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
    from devis_amd import _labelloss
    launches = []
    originals = {name: getattr(_labelloss, name) for name in ("forward", "backward")}
    for name, orig in originals.items():
        setattr(_labelloss, name, lambda *a, _orig=orig, _name=name: launches.append(_name) or _orig(*a))
    try:
        with _Count() as mode:
            fn()
    finally:
        for name, orig in originals.items():
            setattr(_labelloss, name, orig)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labelloss_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("labelloss_bench: no GPU; nothing is measured on the CPU")
    import devis_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    class Patched(StockCriterion):
        pass

    devis_amd.patch_label_loss(types.SimpleNamespace(SetCriterion=Patched))
    stock, patched = StockCriterion(), Patched()
    rows = []
    for T in TARGETS:
        logits = (2 * torch.randn(1, FRAMES * QUERIES, CLASSES, generator=g)).to(dev).requires_grad_(True)
        labels = torch.randint(0, CLASSES, (T * FRAMES,), generator=g)
        valid = torch.rand(T * FRAMES, generator=g) > 0.2
        out_i, tgt_i = torch.randperm(QUERIES, generator=g)[:T], torch.randperm(T, generator=g)
        frames = torch.arange(FRAMES)
        index_i = (frames[None] * QUERIES + out_i[:, None]).reshape(-1)
        index_j = (frames[None] + tgt_i[:, None] * FRAMES).reshape(-1)
        targets = [{"labels": labels.to(dev), "valid": valid.to(dev)}]
        indices = [(index_i.to(dev), index_j.to(dev), valid[index_j].to(dev))]
        num_boxes = float(max(int(valid.sum()), 1))

        def run(criterion):
            out = criterion.loss_labels_focal({"pred_logits": logits}, targets, indices, num_boxes)      # noqa: B023
            grad, = torch.autograd.grad(out["loss_ce"], logits)                                          # noqa: B023
            return out, grad

        (a, ga), (b, gb) = run(stock), run(patched)
        want, got = float(a["loss_ce"].detach()), float(b["loss_ce"].detach())
        diff = abs(want - got)
        res = compare({"replaced": lambda: run(stock), "patched": lambda: run(patched)}, args.windows, args.iters)      # noqa: B023
        rows.append({"targets": T, "matches": T * FRAMES, "loss_ce_replaced": want, "loss_ce_patched": got,
                     "same_loss_ce": diff <= 1e-4 * max(1.0, abs(want)), "class_error_replaced": float(a["class_error"]),
                     "class_error_patched": float(b["class_error"]), "max_gradient_difference": float((ga - gb).abs().max()),
                     "replaced_over_patched": res["replaced"]["ms"] / res["patched"]["ms"], **res})
        print("T = %2d: loss_labels_focal forward + backward replaced %.3f ms, patched %.3f ms" % (T, res["replaced"]["ms"], res["patched"]["ms"]),
              flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "iters": args.iters,
           "shape": {"frames": FRAMES, "queries": QUERIES, "classes": CLASSES},
           "method": "a window is `iters` calls between device synchronises, by a host clock; windows of the sides alternate; "
                     "medians quoted; counts are per call: ATen operators by torch's dispatch mode, this library's kernel launches, "
                     "device activities of a torch.profiler trace, synchronising calls by torch.cuda.set_sync_debug_mode",
           "loss_labels_focal": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Did the DEFAULT path of devis_amd.deform_conv2d get slower?  Times its forward + backward (grad_input by float atomics)
on the six mask-head layers, N = 60, f32 and bf16, with the package of this tree and with the package of another checkout
(the parent commit, built in its own tree), one fresh process per run, the runs alternating on one machine:

    git worktree add ../parent HEAD~1 && (cd ../parent && python -m devis_amd.build)
    python scripts/dcn_ab.py --parent ../parent [--rounds 4] [--merge profiles/dcn_reproducible.json]

(scripts/ab_bench.sh swaps only the library under one binding; across an ABI change the binding refuses the other
library, so here each side runs its own package.)  Per case it records every run, the parent's run-to-run spread
(max - min over min), this tree's median over the parent's median, and whether that deviation lies within the parent's own
spread of that case; the same for the sum over the cases.  --merge writes the block into that JSON document under
"default_path_against_parent"; without it the block is printed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [(264, 264, 12, 20), (264, 128, 12, 20), (136, 64, 23, 40), (72, 32, 45, 80), (32, 16, 90, 160), (16, 1, 90, 160)]
N, WINDOWS, ITERS = 60, 7, 5


def child(tree):
    """One run: {case: median ms over WINDOWS windows of ITERS steps} with the package found in `tree`."""
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import torch
    import devis_amd
    assert os.path.dirname(os.path.dirname(os.path.realpath(devis_amd.__file__))) == os.path.realpath(tree), devis_amd.__file__
    dev = torch.device("cuda:0")
    res = {}
    for C, Co, H, W in LAYERS:
        for dtype in (torch.float32, torch.bfloat16):
            gen = torch.Generator().manual_seed(C + Co)
            x = torch.randn(N, C, H, W, generator=gen).to(dev, dtype).requires_grad_(True)
            off = (torch.rand(N, 18, H, W, generator=gen) * 4 - 2).to(dev).requires_grad_(True)
            msk = (torch.rand(N, 9, H, W, generator=gen) * 2).to(dev).requires_grad_(True)
            w = (torch.randn(Co, C, 3, 3, generator=gen) / (C * 9) ** 0.5).to(dev, dtype).requires_grad_(True)
            g = torch.randn(N, Co, H, W, generator=gen).to(dev, dtype)

            def step():
                out = devis_amd.deform_conv2d(x, off, w, None, 1, 1, 1, msk)
                torch.autograd.grad(out, [x, off, msk, w], g)

            for _ in range(3):
                step()
            torch.cuda.synchronize()
            seen = []
            for _ in range(WINDOWS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(ITERS):
                    step()
                b.record()
                b.synchronize()
                seen.append(a.elapsed_time(b) / ITERS)
            res["C%d->%d %dx%d %s" % (C, Co, H, W, str(dtype).replace("torch.", ""))] = round(statistics.median(seen), 4)
    print(json.dumps(res))


def compare(parent, this):
    """parent / this: lists of runs ({case: ms}) -> the block."""
    def entry(p, t):
        spread = (max(p) - min(p)) / min(p)
        dev = statistics.median(t) / statistics.median(p) - 1
        return {"parent_ms": p, "this_tree_ms": t, "parent_run_to_run": round(spread, 4), "this_over_parent": round(1 + dev, 4),
                "within_parent_run_to_run": abs(dev) <= spread, "slower_beyond_parent_run_to_run": dev > spread}
    rows = [dict(case=k, **entry([r[k] for r in parent], [r[k] for r in this])) for k in parent[0]]
    total = entry([round(sum(r.values()), 4) for r in parent], [round(sum(r.values()), 4) for r in this])
    return {"what": "scripts/dcn_ab.py: default forward + backward, median of %d windows of %d steps per run, one process per "
                    "run, runs alternating parent / this tree on one machine (who goes first alternates by round), each side with "
                    "its own package and library"
                    % (WINDOWS, ITERS),
            "rounds": len(parent), "sum_over_cases": total, "rows": rows,
            "cases_slower_beyond_parent_run_to_run": [r["case"] for r in rows if r["slower_beyond_parent_run_to_run"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the commit to compare with, its library built")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    if not args.parent:
        ap.error("--parent is required")
    runs = {"parent": [], "this": []}
    for i in range(args.rounds):
        # who goes first alternates from round to round: whatever the earlier run leaves behind hits both sides alike
        for side, tree in (("parent", args.parent), ("this", HERE))[::-1 if i % 2 else 1]:
            # a fresh process each: a run that fails or exceeds its limit raises here and nothing more is started
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], stdout=subprocess.PIPE,
                                  timeout=240, check=True)
            runs[side].append(json.loads(done.stdout.decode().strip().splitlines()[-1]))
            print(side, json.dumps(runs[side][-1]), flush=True)
    block = compare(runs["parent"], runs["this"])
    if args.merge:
        with open(args.merge) as f:
            doc = json.load(f)
        doc["default_path_against_parent"] = block
        with open(args.merge, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({k: v for k, v in block.items() if k != "rows"}, indent=1))


if __name__ == "__main__":
    main()

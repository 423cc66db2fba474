"""bench.py --dump-outputs DIR: what the last timed step computed lands in DIR/<name>.npy (float32, within bench.DUMP_BYTES,
large arrays as a fixed, seeded sample) so that two builds can be compared output for output.  CPU: bench.dump_outputs on
host tensors shaped like a step's results; the GPU run of bench.py itself is what writes them for real."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ["out"] + ["grad_" + n for n in bench.LEAF_NAMES]


def _step_results(seed, big=False, clips=1):
    """(outs, grads) as a step returns them: one output per clip, the five leaf gradients per clip in LEAF_NAMES order."""
    g = torch.Generator().manual_seed(seed)
    T, q, M, D, L, P, W, S = 3, 10, 8, 32, 2, 4, 2, 40
    if big:
        S = bench.DUMP_BYTES // 4 // len(NAMES) // (T * M * D) + 7       # grad_value above its share
    outs, grads = [], []
    for _ in range(clips):
        outs.append(torch.randn(T, q, M * D, generator=g))
        grads += [torch.randn(T, S, M, D, generator=g).to(torch.bfloat16), torch.randn(T, q, M, L, P, 2, generator=g),
                  torch.randn(T, q, M, L, P, generator=g), torch.randn(T, q, M, W * L, P, 2, generator=g),
                  torch.randn(T, q, M, W * L, P, generator=g)]
    return outs, tuple(grads)


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}, json.load(open(os.path.join(d, "manifest.json")))


def test_small_outputs_are_written_whole_in_float32(tmp_path):
    outs, grads = _step_results(1)
    bench.dump_outputs(str(tmp_path), outs, grads)
    got, man = _load(str(tmp_path))
    want = dict(zip(NAMES, outs + list(grads)))
    for n in NAMES:
        assert got[n].dtype == np.float32 and not man["arrays"][n]["sampled"]
        assert np.array_equal(got[n], want[n].float().numpy()), n
    assert man["arrays"]["grad_value"]["dtype"] == "bfloat16"


def test_a_large_output_is_a_fixed_seeded_sample_within_the_budget(tmp_path):
    outs, grads = _step_results(2, big=True)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), outs, grads)
    bench.dump_outputs(str(b), outs, grads)
    assert sum(os.path.getsize(os.path.join(a, n + ".npy")) for n in NAMES) <= bench.DUMP_BYTES + 4096
    ga, man = _load(str(a))
    gb, _ = _load(str(b))
    for n in NAMES:
        assert np.array_equal(ga[n], gb[n]), n                       # same inputs -> the same file, sample included
    entry = man["arrays"]["grad_value"]
    share = bench.DUMP_BYTES // 4 // len(NAMES)
    assert entry["sampled"] and entry["shape"] == list(grads[0].shape) and ga["grad_value"].shape == (share,)
    flat = grads[0].float().reshape(-1).numpy()
    runs = np.arange(share + 1, dtype=np.int64) * flat.size // share
    # every sampled value is an element of its own run of the flat array, the runs in order
    for j in (0, 1, share // 2, share - 1):
        assert ga["grad_value"][j] in flat[runs[j]:runs[j + 1]]
    # another tensor of the same size is sampled at the same positions
    other = _step_results(3, big=True)
    c = tmp_path / "c"
    bench.dump_outputs(str(c), *other)
    gc, _ = _load(str(c))
    idx = [int(np.flatnonzero(flat[runs[j]:runs[j + 1]] == ga["grad_value"][j])[0]) + runs[j] for j in (0, share - 1)]
    oflat = other[1][0].float().reshape(-1).numpy()
    assert [gc["grad_value"][0], gc["grad_value"][share - 1]] == [oflat[idx[0]], oflat[idx[1]]]


def test_sharded_results_are_concatenated_clip_by_clip(tmp_path):
    outs, grads = _step_results(4, clips=2)
    bench.dump_outputs(str(tmp_path), outs, grads)
    got, _ = _load(str(tmp_path))
    assert np.array_equal(got["out"], torch.cat(outs, 0).numpy())
    for i, n in enumerate(bench.LEAF_NAMES):
        assert np.array_equal(got["grad_" + n], torch.cat([grads[i], grads[i + 5]], 0).float().numpy()), n


def test_bench_refuses_zero_steps():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr and not r.stdout.strip()

"""CPU: the direction in which the resident-slab gather pass takes its workgroups (GatherPlan::walk_down, csrc/msda_plan.hip), read
from tests/walk_probe.cpp -- the planner as plain C++ under ASan + UBSan, its own process, as tests/test_plan_cpu.py runs its probe.

1. "down" for the bench batch (16 clips of 6 frames, 300 queries, the 360x640 pyramid) in every dtype, and exactly where the call's
   footprint -- value + sampling points + out -- passes kWalkDownBytes;
2. "up" for one clip, for the 60-query call and for the encoder-shaped calls of tests/route_cases.py;
3. nothing else moves: every other field of the plans of the audited shapes is the same with the direction left to the rule, forced
   up and forced down (MSDA_WALK), and a gather pass that is not the resident-slab kernel never walks down.
"""
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT
from route_cases import PYR, TEMPORAL_CALL_ROUTES

CSRC = os.path.join(ROOT, "devis_amd", "csrc")
DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 2, torch.float16: 3}      # include/msda.h, msda_dtype
HOOKS = {"MSDA_ENABLE_HOOKS": "1"}
LIMIT = 256 << 20                                                        # kWalkDownBytes (csrc/msda_params.h)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if not cxx:
        raise RuntimeError("no host C++ compiler (c++, or ROCm's clang++): cannot build tests/walk_probe.cpp")
    exe = str(tmp_path_factory.mktemp("walk_probe") / "walk_probe")
    gcc = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-x", "c++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "walk_probe.cpp"),
           os.path.join(CSRC, "msda_plan.hip"), os.path.join(CSRC, "msda_knobs.hip"), "-o", exe]
    cmd += ["-static-libasan", "-static-libubsan"] if gcc else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(lines, env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MSDA_")}
        clean.update(env or {})
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=clean)
        assert r.returncode == 0 and not r.stderr, "sanitizer report or crash:\n" + r.stderr[-4000:]
        out = [dict(f.split("=", 1) for f in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines) and not any("error" in o for o in out), (lines, r.stdout)
        return out
    return run


def call(dtype=torch.float32, clips=16, frames=6, window=5, Lq=300, pyr="A", cus=256):
    shapes = PYR[pyr]
    Lq = sum(h * w for h, w in shapes) if Lq is None else Lq
    return "%d %d %d %d %d %d %s" % (DTYPE_CODE[dtype], clips, frames, window, Lq, cus, ",".join("%dx%d" % hw for hw in shapes))


def footprint(dtype, clips, frames, window, Lq, pyr, M=8, D=32, P=4):
    """value + sampling locations and weights + out of one call, in bytes (16-bit calls: 16-bit points, as the codes above say)."""
    esz = 4 if dtype == torch.float32 else 2
    S, L = sum(h * w for h, w in PYR[pyr]), len(PYR[pyr])
    points = L * P + window * L * P
    return clips * frames * M * (S * D * esz + Lq * (3 * points * esz + D * esz))


@pytest.mark.parametrize("dtype", list(DTYPE_CODE), ids=lambda d: str(d).replace("torch.", ""))
def test_bench_batch_walks_down(probe, dtype):
    b = probe([call(dtype)])[0]
    assert b["fast"] == "1" and b["gather"] == "2" and b["walk"] == "down", b
    assert int(b["footprint"]) == footprint(dtype, 16, 6, 5, 300, "A") > LIMIT == int(b["limit"]), b


def test_direction_turns_where_the_footprint_passes_the_limit(probe):
    """fp32, 300 queries, the 360x640 pyramid: 48 MB per clip, so 5 clips fit the 256 MiB and 6 do not."""
    per_clip = footprint(torch.float32, 1, 6, 5, 300, "A")
    assert 5 * per_clip <= LIMIT < 6 * per_clip
    out = probe([call(clips=n) for n in range(1, 9)])
    assert [b["walk"] for b in out] == ["up"] * 5 + ["down"] * 3, out
    assert [int(b["footprint"]) for b in out] == [n * per_clip for n in range(1, 9)]


def test_small_and_encoder_shaped_calls_walk_up(probe):
    lines = [call(clips=1), call(clips=1, Lq=60), call(torch.float16, clips=1, Lq=180, pyr="S")]
    lines += [call(dtype, clips=n, Lq=None, pyr=pyr) for pyr, n, lq, dtype, _, _ in TEMPORAL_CALL_ROUTES if lq is None]
    assert len(lines) == 3 + 4
    for line, b in zip(lines, probe(lines)):
        assert b["fast"] == "1" and b["walk"] == "up" and b["knob_walk"] == "-1", (line, b)
    # ... the encoder-shaped ones by their shape, not by their size: one clip of one query per pixel is past the limit
    assert int(probe([call(clips=1, Lq=None)])[0]["footprint"]) > LIMIT


def test_only_the_direction_moves(probe):
    """The plans of every audited temporal call, with the rule, forced up and forced down: the same fields, one by one, except the
    direction (and the knob that forced it); forced down reaches the resident-slab gather pass alone."""
    lines = [call(dtype, clips=n, Lq=lq, pyr=pyr) for pyr, n, lq, dtype, _, _ in TEMPORAL_CALL_ROUTES]
    rule, up, down = probe(lines), probe(lines, {**HOOKS, "MSDA_WALK": "0"}), probe(lines, {**HOOKS, "MSDA_WALK": "1"})
    for line, r, u, d in zip(lines, rule, up, down):
        rest = lambda b: {k: v for k, v in b.items() if k not in ("walk", "knob_walk")}
        assert rest(r) == rest(u) == rest(d) and len(rest(r)) >= 17, (line, r, u, d)
        assert u["walk"] == "up" and d["walk"] == ("down" if d["gather"] == "2" else "up"), (line, u, d)
        assert (r["knob_walk"], u["knob_walk"], d["knob_walk"]) == ("-1", "0", "1")
    assert {d["gather"] for d in down} == {"1", "2"}          # (window and slab gather passes are both among the audited calls)
    # without MSDA_ENABLE_HOOKS=1 the variable is not read
    assert probe(lines, {"MSDA_WALK": "1"}) == rule

"""CPU: the route planner (devis_amd/csrc/msda_plan.hip, msda_knobs.hip) run as plain C++ under ASan + UBSan.

tests/plan_probe.cpp is built once per session with the HOST compiler, the sanitizers on and no ROCm include path -- that it
builds is the proof that both units are free of HIP -- and every test feeds it call shapes and reads the plans it prints.  The
probe is its own process with the sanitizer runtimes linked in: nothing here loads one into python.

1. the shapes of tests/route_cases.py get, at 256 CUs, the plan their GPU labels name (tests/test_routes_gpu.py);
2. every 32-bit guard of the planner is crossed once: a shape just inside it and one just outside it, the limits as the code
   writes them.  Nothing is allocated, so the shapes are as large as the guards require;
3. the knobs: environment over pin, unknown pin names, the two halves of MSDA_SCATTER_DBG.
"""
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT
from route_cases import PYR, SINGLE_FRAME_FORWARD_ROUTES, TEMPORAL_CALL_ROUTES

CSRC = os.path.join(ROOT, "devis_amd", "csrc")
DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 2, torch.float16: 3}      # include/msda.h, msda_dtype
HOOKS = {"MSDA_ENABLE_HOOKS": "1"}


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if not cxx:
        raise RuntimeError("no host C++ compiler (c++, or ROCm's clang++): cannot build tests/plan_probe.cpp")
    exe = str(tmp_path_factory.mktemp("plan_probe") / "plan_probe")
    # (gcc links the sanitizer runtimes as shared objects unless told otherwise, clang statically: static either way, so that the
    # probe carries its runtimes and starts whatever else the environment loads into a process)
    gcc = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-x", "c++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "plan_probe.cpp"),
           os.path.join(CSRC, "msda_plan.hip"), os.path.join(CSRC, "msda_knobs.hip"), "-o", exe]
    cmd += ["-static-libasan", "-static-libubsan"] if gcc else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(lines, env=None):
        """One probe process over `lines`; the MSDA_* variables of the caller's environment are replaced by `env`."""
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MSDA_")}
        clean.update(env or {})
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=clean)
        assert r.returncode == 0 and not r.stderr, "sanitizer report or crash:\n" + r.stderr[-4000:]      # a finding, not noise
        out = [dict(f.split("=", 1) for f in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines) and not any("error" in o for o in out), (lines, r.stdout)
        return out
    return run


def shape(direction="f", dtype=0, clips=1, frames=1, window=0, S=None, M=8, D=32, L=None, Lq=300, Pc=4, Pt=4, cus=256, shapes=None,
          grads=3, vs=None, cmd="shape"):
    """One line of the probe.  `shapes`: [(H, W), ...] -- S and L default to what it holds -- or None: no host copy."""
    if shapes is not None:
        S = sum(h * w for h, w in shapes) if S is None else S
        L = len(shapes) if L is None else L
    text = ",".join("%dx%d" % hw for hw in shapes) if shapes is not None else "-"
    line = "%s %s %d %d %d %d %d %d %d %d %d %d %d %d %s %d" % (cmd, direction, dtype, clips, frames, window, S, M, D, L, Lq, Pc, Pt, cus, text, grads)
    return line + (" vs=%d,%d,%d" % vs if vs else "")


# ---- 1. the audited shapes -----------------------------------------------------------------------------------------------

def forward_plan_is(label, f):
    if label == "(tile kernel)":
        return f["family"] == "tile" and f["waves"] == "1"
    if label == "tile kernel, several waves per tile":
        return f["family"] == "tile" and int(f["waves"]) > 1
    if label == "tile kernel":
        return f["family"] == "tile"
    if label.startswith("resident-slab kernel, ") and label.endswith(" tiles per wave"):
        return f["family"] == "slab" and f["nt"] == label.split()[2]
    return {"resident-slab kernel": "slab", "resident-window kernel": "window"}[label] == f["family"]


def gather_plan_is(label, b):
    want = {"one source frame per workgroup": ("slab", "1"), "resident-slab kernel, grad_loc/grad_attn)": ("slab", "0"),
            "resident-window kernel": ("window", "0")}[label]
    return (b["gather"], b["frame_split"]) == want


@pytest.mark.parametrize("pyr,clips,Lq,dtype,fwd_has,bwd_has", TEMPORAL_CALL_ROUTES,
                         ids=lambda v: str(v).replace("torch.", "") if not isinstance(v, str) or len(v) < 3 else None)
def test_temporal_call_plans(probe, pyr, clips, Lq, dtype, fwd_has, bwd_has):
    S = sum(h * w for h, w in PYR[pyr])
    call = dict(dtype=DTYPE_CODE[dtype], clips=clips, frames=6, window=5, Lq=S if Lq is None else Lq, shapes=PYR[pyr])
    f, b = probe([shape("f", **call), shape("b", **call)])
    assert f["fast"] == b["fast"] == "1" and f["too_large"] == b["too_large"] == "0", (f, b)
    assert forward_plan_is(fwd_has, f), f
    assert gather_plan_is(bwd_has, b), b
    # "owner-computes scatter" in the route and no "zero-fill": the zero-fill rides in the scatter kernel
    assert b["scatter"] == "owner" and b["run_owner"] == "1" and b["fused_zero"] == "1", b


def test_single_frame_decoder_like_forward_plans(probe):
    out = probe([shape("f", DTYPE_CODE[dtype], clips=n, Lq=lq, shapes=PYR[pyr]) for pyr, n, lq, dtype, _ in SINGLE_FRAME_FORWARD_ROUTES])
    for (_, _, _, _, label), f in zip(SINGLE_FRAME_FORWARD_ROUTES, out):
        assert f["fast"] == "1" and forward_plan_is(label, f), (label, f)


# ---- 2. the 32-bit guards ------------------------------------------------------------------------------------------------
# (field, inside shape, outside shape, value inside, value outside[, environment]); every pair differs in ONE size, by the least
# step that crosses the limit.  TINY: a one-level pyramid where the sizes under test are the only large ones.
TINY = [(4, 5)]
MFMA = {**HOOKS, "MSDA_SCATTER_MFMA": "1"}         # the matrix-pipe levels wherever they apply: the guard alone decides
GUARDS = {
    # shape_of: workgroups of the tile kernels, groups * ceil(Lq / 8) * M, > 0x7fffffff (a prime: one head, 8 queries)
    "shape_of blocks": ("too_large", shape(clips=0x7fffffff, M=1, Lq=8, shapes=TINY), shape(clips=1 << 30, M=1, Lq=16, shapes=TINY), "0", "1"),
    # rs_fits (strides through value_strides, so that one term moves at a time)
    "rs_fits frames*S < 2^24": ("rs_fits", shape(S=(1 << 24) - 1, L=1, vs=(0, 32, 4)), shape(S=1 << 24, L=1, vs=(0, 32, 4)), "1", "0"),
    "rs_fits pixB < 2^24": ("rs_fits", shape(S=20, L=1, vs=(0, 32, (1 << 22) - 1)), shape(S=20, L=1, vs=(0, 32, 1 << 22)), "1", "0"),
    "rs_fits frames*S*pixB < 0x7fffffff": ("rs_fits", shape(S=(1 << 23) - 1, L=1, M=2), shape(S=1 << 23, L=1, M=2), "1", "0"),
    "rs_fits frames <= 32": ("rs_fits", shape(frames=32, shapes=TINY), shape(frames=33, shapes=TINY), "1", "0"),
    "rs_fits window <= 31": ("rs_fits", shape(frames=32, window=31, shapes=TINY), shape(frames=32, window=32, shapes=TINY), "1", "0"),
    # scatter_applicable: 2147483646 = 198 * 10845877
    "scatter groups*Lq < 0x7fffffff": ("scatter_ok", shape("b", clips=198, M=1, Lq=10845877, shapes=TINY),
                                       shape("b", clips=198, M=1, Lq=10845878, shapes=TINY), "1", "0"),
    "scatter Lq < 2^24": ("scatter_ok", shape("b", M=1, Lq=(1 << 24) - 1, shapes=TINY), shape("b", M=1, Lq=1 << 24, shapes=TINY), "1", "0"),
    "scatter 64 sources": ("scatter_ok", shape("b", frames=9, window=7, shapes=TINY), shape("b", frames=8, window=8, shapes=TINY), "1", "0"),
    # owner_scatter_applicable: groups * M * (S + L), again 198 * 10845877 and one more
    "owner groups*M*(S+L) < 0x7fffffff": ("owner_ok", shape("b", clips=198, M=1, S=10845876, L=1), shape("b", clips=198, M=1, S=10845877, L=1), "1", "0"),
    "owner Lq < 2^22": ("owner_ok", shape("b", M=1, Lq=(1 << 22) - 1, shapes=TINY), shape("b", M=1, Lq=1 << 22, shapes=TINY), "1", "0"),
    # plan_matrix_pipe: a clip's grad_out (rows * M * D * esz) and its point arrays (rows * M * L * P * 2 * 4) below 2 GiB
    "matrix pipe grad_out of a clip": ("mfma_tiles", shape("b", Lq=(1 << 21) - 1, shapes=[(8, 8), (4, 4)]),
                                       shape("b", Lq=1 << 21, shapes=[(8, 8), (4, 4)]), "2", "0", MFMA),
    "matrix pipe points of a clip": ("mfma_tiles", shape("b", 4, Lq=2796202, shapes=[(8, 8), (4, 4), (2, 2)]),
                                     shape("b", 4, Lq=2796203, shapes=[(8, 8), (4, 4), (2, 2)]), "2", "0", MFMA),
    # win_plan: win_axis forms 2 * n_l * n_0 in 32 bits
    "window plan rows": ("win", shape(Lq=16000, shapes=[(16000, 1)]), shape(Lq=16001, shapes=[(16001, 1)]), "1", "0"),
    "window plan columns": ("win", shape(Lq=16000, shapes=[(1, 16000)]), shape(Lq=16001, shapes=[(1, 16001)]), "1", "0"),
    # fast_path_takes: frames * S * M * D elements (the strided twin, frames * S * v_pix, cannot pass 0x7fffffff before its bytes
    # pass kOobBytes in any element size the fast path has, so it has no inside / outside pair of its own)
    "fast path 0x7fffffff elements": ("fast", shape(S=(1 << 23) - 1, L=1, vs=(0, 32, 4)), shape(S=1 << 23, L=1, vs=(0, 32, 4)), "1", "0"),
    "fast path kOobBytes": ("fast", shape(S=0xF0000000 // 128 - 1, L=1, M=1), shape(S=0xF0000000 // 128, L=1, M=1), "1", "0"),
    # plan_gather: (clip, head, frame, part) workgroups; past the limit the (clip, head, part) grid takes over
    "gather frame-split grid": ("frame_split", shape("b", clips=(1 << 29) - 1, frames=2, M=1, Lq=1, shapes=TINY),
                                shape("b", clips=1 << 29, frames=2, M=1, Lq=1, shapes=TINY), "1", "0",
                                {**HOOKS, "MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "2", "MSDA_BWD_CULL": "0"}),
}


@pytest.mark.parametrize("guard", list(GUARDS))
def test_guard_is_crossed_once(probe, guard):
    field, inside, outside, want_in, want_out, *env = GUARDS[guard]
    a, b = probe([inside, outside], *env)
    assert (a.get(field), b.get(field)) == (want_in, want_out), (a, b)


def test_slab_grids_at_their_limit(probe):
    """plan_forward's and plan_gather's (clip, head, part) grids are never larger than the tile kernels' block count, so shape_of
    turns a call away before either limit can be passed: the largest call shape_of lets through still gets the slab kernels (the
    backward one row short of it: groups * Lq of a scatter stays below 0x7fffffff)."""
    env = {**HOOKS, "MSDA_FWD_RS": "1", "MSDA_FWD_RS_NT": "1", "MSDA_BWD_RS": "1", "MSDA_BWD_RS_FSPLIT": "0", "MSDA_BWD_CULL": "0"}
    f, b, over = probe([shape("f", clips=0x7fffffff, M=1, Lq=8, shapes=TINY), shape("b", clips=0x7ffffffe, M=1, Lq=1, shapes=TINY),
                        shape("f", clips=1 << 30, M=1, Lq=16, shapes=TINY)], env)
    assert (f["family"], f["nt"], f["parts"]) == ("slab", "1", "1"), f
    assert (b["gather"], b["frame_split"], b["g_grid"]) == ("slab", "0", str(0x7ffffffe)), b
    assert over["too_large"] == "1" and "family" not in over, over


def test_row_counts_of_the_largest_query_count_are_formed_in_64_bits(probe):
    """UBSan's finding in shape_of: Lq + rows per wave - 1 (and + 15 for the slab kernels' tiles) overflowed an int from
    Lq = 2^31 - 8 on; both are widened.  2^31 - 1 queries of one head are 2^28 workgroups of 8 rows: not too large."""
    f = probe([shape(M=1, Lq=0x7fffffff, shapes=TINY)])[0]
    assert (f["fast"], f["too_large"], f["blocks"]) == ("1", "0", str(1 << 28)), f


# ---- 3. knobs ------------------------------------------------------------------------------------------------------------

def test_environment_wins_over_a_pin_even_at_its_default(probe):
    call = dict(clips=16, frames=6, window=5, shapes=PYR["A"])
    lines = [shape(**call), shape(cmd="pin fwd_rs=0", **call), shape(**call), shape(clips=17, frames=6, window=5, shapes=PYR["A"]),
             shape(cmd="pin -", **call), shape(**call)]
    rules, pinned, with_pin, other_shape, removed, after = probe(lines)
    assert rules["family"] == "slab" and rules["knob_forced"] == "0", rules
    assert (pinned["pinned"], pinned["routes"]) == ("1", "1") and (removed["pinned"], removed["routes"]) == ("1", "0")
    assert with_pin["family"] == "tile" and with_pin["knob_fwd_rs"] == "0", with_pin
    assert other_shape["family"] == "slab" and after == rules
    forced = probe(lines, {**HOOKS, "MSDA_FWD_RS": "-1"})[2]          # set to its default: the rules decide, not the pin
    assert forced["family"] == "slab" and forced["knob_fwd_rs"] == "-1" and forced["knob_forced"] != "0", forced
    assert probe(lines, {"MSDA_FWD_RS": "-1"})[2]["family"] == "tile"        # without MSDA_ENABLE_HOOKS=1 the variable is not read


def test_pin_settings_with_an_unknown_name_are_rejected(probe):
    call = dict(clips=16, frames=6, window=5, shapes=PYR["A"])
    out = probe(["parse fwd_rs=1,fwd_win=0", "parse fwd_rs=1,bogus=2", "parse win_min_halo=3", "parse fwd_rs",
                 shape(cmd="pin fwd_rs=0,bogus=1", **call), shape(**call)])
    assert [o.get("parsed") for o in out[:4]] == ["1", "0", "0", "0"]        # (win_min_halo is a knob, but not a pinnable one)
    assert (out[4]["pinned"], out[4]["routes"]) == ("0", "0") and out[5]["family"] == "slab", out[4:]


@pytest.mark.parametrize("text,order,dbg", [("3", 0, 3), ("259", 1, 3), ("2051", 2, 3), ("2307", 1, 3), ("6656", 2, 4608)])
def test_scatter_dbg_splits_into_order_and_debug_bits(probe, text, order, dbg):
    """knob_value: bit 256 = level order (1), else bit 2048 = image order (2); the other bits are the kernels' debug bits."""
    k = probe([shape(shapes=TINY)], {**HOOKS, "MSDA_SCATTER_DBG": text})[0]
    assert (int(k["knob_scatter_order"]), int(k["knob_scatter_dbg"])) == (order, dbg), k
    off = probe([shape(shapes=TINY)], {"MSDA_SCATTER_DBG": text})[0]           # without MSDA_ENABLE_HOOKS=1: not read
    assert (off["knob_scatter_order"], off["knob_scatter_dbg"]) == ("0", "0"), off


# ---- 4. the table of the measurement bits (csrc/msda_params.h) and its Python twin (devis_amd/tuning.py) ----------------------

def _header_bits():
    """{name: value} of the header's kSdbg* / kDbg* constants and kOwnFusedZero, read as text in file order: a value is a number
    or an expression over the names before it (| & ~ << and parentheses mean the same in Python)."""
    import re
    with open(os.path.join(CSRC, "msda_params.h")) as f:
        text = f.read()
    bits = {}
    for decl in re.findall(r"^constexpr int ((?:kSdbg|kDbg|kOwnFusedZero)[^;]*);", text, re.M):
        for item in decl.split(","):           # (constexpr int a = 1, b = 2;)
            name, expr = (s.strip() for s in item.split("="))
            assert re.fullmatch(r"[\w\s|&~()<]+", expr), item
            bits[name] = eval(expr, {"__builtins__": {}}, dict(bits))
    return bits


def test_bit_names_of_the_tuning_module_are_the_headers():
    """Both directions: every constant of the header's table is in devis_amd/tuning.py with the same value, and the module names
    no bit the header does not."""
    from devis_amd import tuning
    header = _header_bits()
    assert len(header) >= 25 and header["kSdbgStaticStride"] == 16 and header["kOwnFusedZero"] == 512, header
    module = {n: v for n, v in vars(tuning).items() if n.startswith(("kSdbg", "kDbg", "kOwnFusedZero"))}
    assert module == header, (sorted(set(module) ^ set(header)), {n: (module[n], header[n]) for n in set(module) & set(header) if module[n] != header[n]})


def test_bit_groups_are_consistent():
    """A bit of MSDA_SCATTER_DBG is a route bit or an ablation bit, never both; the two masks (the order bits are route bits) cover
    every named bit; the launch flag is no environment bit; the owner kernel is passed no bit only the host reads."""
    b = _header_bits()
    masks = ("kSdbgRouteMask", "kSdbgAblationMask", "kSdbgOrderMask", "kSdbgOwnMask", "kSdbgLdsMask", "kSdbgOwnLevelShift", "kSdbgOwnLevelMask")
    named = 0
    for name, v in b.items():
        if name.startswith("kSdbg") and name not in masks:
            named |= v
    route, ablation, order = b["kSdbgRouteMask"], b["kSdbgAblationMask"], b["kSdbgOrderMask"]
    assert route & ablation == 0
    assert route | ablation | order == named and named == 1 | 2 | 4 | 8 | 16 | 224 | 256 | 1024 | 2048 | 4096 | 8192, (route, ablation, named)
    assert order == 256 | 2048 and b["kSdbgOwnLevelField"] == b["kSdbgOwnLevelMask"] << b["kSdbgOwnLevelShift"] == 224
    assert b["kOwnFusedZero"] == 512 and b["kOwnFusedZero"] & (route | ablation | order) == 0
    host_only = b["kSdbgSeparateZero"] | b["kSdbgNoFourSlotRule"]
    assert host_only == 1024 | 8192 and b["kSdbgOwnMask"] & (host_only | order | b["kOwnFusedZero"]) == 0
    assert b["kSdbgOwnMask"] == 255 | 4096 and b["kSdbgLdsMask"] == 2 | 4 | 8 | 16          # what each kernel tests, by value
    assert b["kSdbgLdsMask"] & (host_only | order | b["kOwnFusedZero"]) == 0
    # MSDA_DBG
    assert b["kDbgRouteMask"] & b["kDbgAblationMask"] == 0
    assert (b["kDbgRouteMask"], b["kDbgAblationMask"]) == (32 | 64 | 128, 8 | 16)
    assert b["kDbgRouteMask"] | b["kDbgAblationMask"] == sum(v for n, v in b.items() if n.startswith("kDbg") and not n.endswith("Mask"))


def test_no_bare_literal_tests_a_debug_word():
    """The project's own source, as text: no `dbg` / `flags` / `scatter_dbg` is tested against a number (& or >>, then a digit)
    in csrc/msda_*.hip and msda_*.h -- every test names its bit."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(CSRC, "msda_*.hip")) + glob.glob(os.path.join(CSRC, "msda_*.h")))
    assert len(files) >= 14, files
    pat = re.compile(r"(?:dbg|flags)\s*(?:&|>>)\s*\(?\s*~?\s*\d")
    hits = []
    for path in files:
        with open(path) as f:
            hits += ["%s:%d: %s" % (os.path.basename(path), i, ln.strip()) for i, ln in enumerate(f, 1) if pat.search(ln)]
    assert not hits, "\n".join(hits)
    assert pat.search("if (dbg & 16)") and pat.search("(k.scatter_dbg & (511 | 4096))") and pat.search("(flags >> 5) & 7")

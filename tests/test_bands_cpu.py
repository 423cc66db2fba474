"""CPU: the band arithmetic of the owner-computes scatter on both sides of its limits.

A band of msda_bwd_value_grp_kernel is 256 owner quads x own_slots(dtype, gv_storage) pixels (devis_amd/csrc/msda_params.h):
five slots -- 1280 pixels -- in fp32 and where a 16-bit grad_value is written in the storage type, four -- 1024 -- for a 16-bit
type with float grad_value.  A level whose row is wider than 1024 pixels is "direct" (float atomics) at either size, as it always
was; any other level of H x W pixels is cut into nb = ceil(H / floor(pix / W)) bands of equal
height to within one row, the H % nb taller ones first.  The kernel, the planner (band count of the image order, the one-band
rule of rec_mask, the fused zero-fill's width test, the width test of a storage-typed grad_value) and the zero-fill all use
own_band_pixels / own_band_count / own_band_rows: every case below is checked against the band list computed here in plain
Python, through the planner probe of tests/test_plan_cpu.py (which takes grad_value in the type the library names: fp32 and the
five-slot 16-bit calls) and through tests/band_probe.cpp (which takes gv_storage as an input and prints the rows the device forms).
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from devis_amd.tuning import kSdbgImageOrder, kSdbgNoFourSlotRule        # MSDA_SCATTER_DBG bits by name (csrc/msda_params.h)
from test_plan_cpu import CSRC, HOOKS, probe, shape      # noqa: F401  (probe: the session's planner probe, a fixture)

F32, BF16, F16, BF16_LOC32, F16_LOC32 = 0, 2, 3, 4, 5        # include/msda.h, msda_dtype
QUADS = 256                                                  # owner quads of a workgroup (kOwnThreads / 4)
ROW_LIMIT = 1024                                             # a wider row is "direct" whatever the slots (kOwnPix)


def slots(dtype, gv_storage):
    return 5 if dtype == F32 or gv_storage else 4


def bands(H, W, pix):
    """[(first row, last row), ...] of a level, or None for a "direct" level (a row wider than a band)."""
    per = pix // W
    if per == 0 or W > ROW_LIMIT:
        return None
    nb = 1 if per >= H else -(-H // per)
    q, rem = divmod(H, nb)
    out, r = [], 0
    for b in range(nb):
        h = q + (1 if b < rem else 0)
        out.append((r, r + h - 1))
        r += h
    assert r == H and max(h1 - h0 for h0, h1 in out) - min(h1 - h0 for h0, h1 in out) <= 1
    assert all((h1 - h0 + 1) * W <= pix for h0, h1 in out)
    return out


@pytest.fixture(scope="module")
def band_probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if not cxx:
        raise RuntimeError("no host C++ compiler (c++, or ROCm's clang++): cannot build tests/band_probe.cpp")
    exe = str(tmp_path_factory.mktemp("band_probe") / "band_probe")
    gcc = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-x", "c++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "band_probe.cpp"),
           os.path.join(CSRC, "msda_plan.hip"), os.path.join(CSRC, "msda_knobs.hip"), "-o", exe]
    cmd += ["-static-libasan", "-static-libubsan"] if gcc else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(calls, env=None):
        """calls: (dtype, gv_storage, shapes[, Lq, clips, frames, window]) -> one dict of fields per call."""
        lines = []
        for dtype, gv, shapes, *rest in calls:
            Lq, clips, frames, window = (list(rest) + [300, 16, 6, 5][len(rest):])
            lines.append("%d %d %d %d %d %d %s" % (dtype, gv, clips, frames, window, Lq, ",".join("%dx%d" % hw for hw in shapes)))
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MSDA_")}
        clean.update(env or {})
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=clean)
        assert r.returncode == 0 and not r.stderr, "sanitizer report or crash:\n" + r.stderr[-4000:]
        out = [dict(f.split("=", 1) for f in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines) and not any("error" in o for o in out), (lines, r.stdout)
        return out
    return run


def rows_text(shapes, pix):
    return "|".join("direct" if bands(h, w, pix) is None else ";".join("%d-%d" % b for b in bands(h, w, pix)) for h, w in shapes)


def count_text(shapes, pix):
    return ",".join(str(0 if bands(h, w, pix) is None else len(bands(h, w, pix))) for h, w in shapes)


# ---- the device's rows ------------------------------------------------------------------------------------------------------

def test_the_expected_band_lists_themselves():
    """The plain-Python list at the sizes the design names."""
    assert [b - a + 1 for a, b in bands(45, 80, 1280)] == [15, 15, 15]
    assert [b - a + 1 for a, b in bands(45, 80, 1024)] == [12, 11, 11, 11]
    assert [b - a + 1 for a, b in bands(33, 80, 1280)] == [11, 11, 11]
    assert [b - a + 1 for a, b in bands(17, 80, 1280)] == [9, 8]
    assert [b - a + 1 for a, b in bands(7, 400, 1280)] == [3, 2, 2]          # 3 rows per band, a height they do not divide
    assert bands(16, 80, 1280) == [(0, 15)] and len(bands(17, 80, 1280)) == 2
    assert bands(25, 42, 1280) == [(0, 24)] and len(bands(25, 42, 1024)) == 2
    assert bands(3, 1281, 1280) is None and bands(3, 1280, 1280) is None and bands(3, 1025, 1280) is None
    assert bands(3, 1024, 1280) == [(0, 0), (1, 1), (2, 2)] == bands(3, 1024, 1024) and bands(3, 1025, 1024) is None
    assert [b - a + 1 for a, b in bands(5, 640, 1280)] == [2, 2, 1] and len(bands(5, 640, 1024)) == 5


LEVELS = [(45, 80), (25, 42), (16, 80), (17, 80), (33, 80), (7, 400), (7, 341), (3, 1280), (3, 1281), (3, 1024), (3, 1025), (5, 640), (1, 1),
          (1300, 1), (100, 167), (50, 84), (23, 40), (2000, 3)]


@pytest.mark.parametrize("dtype,gv", [(F32, 0), (BF16, 1), (F16, 1), (BF16_LOC32, 1), (F16_LOC32, 1),
                                      (BF16, 0), (F16, 0), (BF16_LOC32, 0), (F16_LOC32, 0)])
def test_device_rows_match_the_plain_python_list(band_probe, dtype, gv):
    """own_slots per (dtype, gv_storage), and per level the band count and every band's first and last row as the kernel forms
    them (32-bit, H / nb and H % nb), equal to the planner's 64-bit count (the probe reports a mismatch as an error)."""
    pix = QUADS * slots(dtype, gv)
    # one call per level (a pyramid may hold a direct level only with float grad_value; the rows do not depend on the rest)
    out = band_probe([(dtype, gv, [hw, (6, 10)]) for hw in LEVELS])
    for hw, o in zip(LEVELS, out):
        assert (int(o["slots"]), int(o["pix"])) == (slots(dtype, gv), pix), o
        assert o["bands"] == count_text([hw, (6, 10)], pix) and o["rows"] == rows_text([hw, (6, 10)], pix), (hw, o)


# ---- the planner -------------------------------------------------------------------------------------------------------------

def bit(o, l):
    return (int(o["rec_mask"]) >> l) & 1


def test_one_band_rule_of_rec_mask_on_both_sides_of_both_limits(band_probe):
    """A level of one band leaves no culling records.  25 x 42 = 1050 pixels: one band at five slots, two at four; 16 x 80 = 1280
    is one band at five slots and 17 x 80 two; 12 x 80 / 13 x 80 are the same pair at four slots.  The matrix pipe is off, so
    that every level is the owner kernel's."""
    env = {**HOOKS, "MSDA_SCATTER_MFMA": "0"}
    pyr = [(45, 80), (25, 42), (16, 80), (17, 80), (12, 80), (13, 80)]
    for dtype, gv in [(F32, 0), (BF16, 1), (BF16_LOC32, 1), (BF16, 0), (F16_LOC32, 0)]:
        pix = QUADS * slots(dtype, gv)
        o = band_probe([(dtype, gv, pyr)], env)[0]
        assert o["owner"] == "1" and int(o["sc_l0"]) == len(pyr), o
        want = [0 if len(bands(h, w, pix)) == 1 else 1 for h, w in pyr]
        assert [bit(o, l) for l in range(len(pyr))] == want, (dtype, gv, o)
        assert want == ([1, 0, 0, 1, 0, 0] if pix == 1280 else [1, 1, 1, 1, 0, 1])
        assert o["bands"] == ("3,1,1,2,1,1" if pix == 1280 else "4,2,2,2,1,2"), o


def test_same_rule_through_the_planner_probe(probe):
    """tests/plan_probe.cpp, grad_value in the type the library names: fp32 (five slots) and bf16 in the storage type (five slots)
    clear the bit of the 800x1333 pyramid's 25 x 42 level; the 50 x 84 level above it keeps its records."""
    pyr = [(100, 167), (50, 84), (25, 42), (13, 21)]
    env = {**HOOKS, "MSDA_SCATTER_MFMA": "0"}
    for dtype in (F32, BF16, BF16_LOC32):
        b = probe([shape("b", dtype, clips=16, frames=6, window=5, shapes=pyr)], env)[0]
        assert b["scatter"] == "owner" and b["gv_storage"] == ("0" if dtype == F32 else "1"), b
        assert [(int(b["rec_mask"]) >> l) & 1 for l in range(4)] == [1, 1, 0, 0], b


def test_width_limit_of_the_fused_zero_fill_and_of_a_storage_typed_grad_value(probe, band_probe):
    """A row of 1024 pixels fits a band and 1025 is "direct" (float atomics: a zero-fill launch of its own, and grad_value in
    the arithmetic type) in EVERY instantiation: the fifth slot makes bands taller, not rows wider.  1280 and 1281, on both sides
    of a five-slot band's pixel count, are direct alike."""
    for dtype, gv in [(F32, 0), (BF16, 1), (BF16, 0), (F16_LOC32, 0)]:
        a, b, c, d = band_probe([(dtype, gv, [(3, w), (3, 5)]) for w in (1024, 1025, 1280, 1281)])
        assert [x["fused_zero"] for x in (a, b, c, d)] == ["1", "0", "0", "0"], (a, b, c, d)
        assert [x["bands"] for x in (a, b, c, d)] == ["3,1", "0,1", "0,1", "0,1"], (a, b, c, d)
        assert [x["gv_ok"] for x in (a, b, c, d)] == (["1", "0", "0", "0"] if dtype != F32 else ["0"] * 4), (a, b, c, d)
    # ... and through the planner probe: fp32 and bf16
    f0, f1, f2, h0, h1 = probe([shape("b", F32, shapes=[(3, 1024), (3, 5)]), shape("b", F32, shapes=[(3, 1025), (3, 5)]),
                                shape("b", F32, shapes=[(3, 1281), (3, 5)]),
                                shape("b", BF16, shapes=[(3, 1024), (3, 5)]), shape("b", BF16, shapes=[(3, 1025), (3, 5)])])
    assert (f0["fused_zero"], f1["fused_zero"], f2["fused_zero"]) == ("1", "0", "0"), (f0, f1, f2)
    assert (h0["gv_storage"], h0["fused_zero"], h1["gv_storage"], h1["fused_zero"]) == ("1", "1", "0", "0"), (h0, h1)


def test_band_count_of_the_image_order(band_probe):
    """owner_image_order sorts up to 256 (level, band) pairs: a tall level beside the 45 x 80 one puts the total on both sides of
    it, which counts the 45 x 80 level's own bands -- 3 at five slots, 4 at four."""
    env = {**HOOKS, "MSDA_SCATTER_DBG": str(kSdbgImageOrder), "MSDA_SCATTER_MFMA": "0"}            # image order wherever the bands can be sorted
    for dtype, gv in [(F32, 0), (BF16, 1), (BF16, 0), (F16_LOC32, 0)]:
        pix = QUADS * slots(dtype, gv)
        per = pix // 80
        n45 = len(bands(45, 80, pix))
        assert n45 == (3 if pix == 1280 else 4)
        tall = (256 - n45) * per                                          # 256 - n45 bands exactly
        assert len(bands(tall, 80, pix)) == 256 - n45 and len(bands(tall + 1, 80, pix)) == 257 - n45
        a, b = band_probe([(dtype, gv, [(45, 80), (tall, 80)]), (dtype, gv, [(45, 80), (tall + 1, 80)])], env)
        assert (a["image_order"], b["image_order"]) == ("1", "0"), (dtype, gv, a, b)
        assert a["bands"] == "%d,%d" % (n45, 256 - n45), a


# ---- the planner's choice per call ---------------------------------------------------------------------------------------------

PYR_A = [(45, 80), (23, 40), (12, 20), (6, 10)]


def test_few_item_calls_stay_on_four_slots(band_probe):
    """plan_scatter: a call of at most two items per workgroup of the persistent grid (256 at 256 CUs), counted at five slots,
    keeps 1024-pixel bands -- its launch lasts as long as its heaviest band; larger calls take what own_slots allows.  One clip
    of the decoder call is 6 x 8 x (3 + 1 + 1 + 1) = 288 items, two clips 576.  MSDA_SCATTER_DBG kSdbgNoFourSlotRule switches the rule off."""
    one, two, many, half = band_probe([(F32, 0, PYR_A, 300, 1), (F32, 0, PYR_A, 300, 2), (F32, 0, PYR_A, 300, 16), (BF16, 1, PYR_A, 300, 1)])
    assert [o["own_pix"] for o in (one, two, many, half)] == ["1024", "1280", "1280", "1024"], (one, two, many, half)
    forced = band_probe([(F32, 0, PYR_A, 300, 1), (BF16, 1, PYR_A, 300, 1), (BF16, 0, PYR_A, 300, 16)], {**HOOKS, "MSDA_SCATTER_DBG": str(kSdbgNoFourSlotRule)})
    assert [o["own_pix"] for o in forced] == ["1280", "1280", "1024"], forced          # (four is all a float grad_value beside bf16 has)
    # the boundary: one level of 45 x 80 (3 bands at five slots), single-frame calls of c images: 24 c items against 512
    a, b = band_probe([(F32, 0, [(45, 80)], 300, 21, 1, 0), (F32, 0, [(45, 80)], 300, 22, 1, 0)])
    assert (a["own_pix"], b["own_pix"]) == ("1024", "1280"), (a, b)


def test_every_band_count_follows_the_chosen_size(band_probe):
    """The one-band rule of rec_mask is evaluated at the size the planner chose, which is the size of the kernel it launches
    (Params::own_pix): 25 x 42 in a two-frame call of one clip is two bands of 1024 pixels and keeps its records; with the
    few-item rule off it is one band of 1280 and leaves none."""
    env = {**HOOKS, "MSDA_SCATTER_MFMA": "0"}
    call = (F32, 0, [(25, 42), (13, 21)], 40, 1, 2, 1)
    small = band_probe([call], env)[0]
    forced = band_probe([call], {**env, "MSDA_SCATTER_DBG": str(kSdbgNoFourSlotRule)})[0]
    assert (small["own_pix"], bit(small, 0), bit(small, 1)) == ("1024", 1, 0), small
    assert (forced["own_pix"], bit(forced, 0), bit(forced, 1)) == ("1280", 0, 0), forced
    for o in (small, forced):
        want = [0 if len(bands(h, w, int(o["own_pix"]))) == 1 else 1 for h, w in [(25, 42), (13, 21)]]
        assert [bit(o, 0), bit(o, 1)] == want, o

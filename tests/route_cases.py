"""Call shapes whose route the rules must keep, with the substrings of msda_last_route that name it: shared by
tests/test_routes_gpu.py (the labels of the kernels launched on the GPU) and tests/test_plan_cpu.py (the plan the same rules make on
a CPU, csrc/msda_plan.hip).  Every shape has 8 heads of 32 channels, 4 levels and 4 points per level."""
import torch

PYR = {"A": [(45, 80), (23, 40), (12, 20), (6, 10)], "S": [(60, 96), (30, 48), (15, 24), (8, 12)], "B": [(100, 167), (50, 84), (25, 42), (13, 21)]}

# Fused temporal calls of 6 frames: (pyramid, clips, queries per frame -- None: one per pixel --, dtype, forward label, backward label)
TEMPORAL_CALL_ROUTES = [
    # the call DeVIS issues: tile forward, gather pass on the slab kernel with the frames as a workgroup index
    ("A", 1, 300, torch.float32, "(tile kernel)", "one source frame per workgroup"),
    ("B", 1, 300, torch.bfloat16, "tile kernel", "one source frame per workgroup"),
    # ... at the query counts of DeVIS's shipped configs (60 per frame on YouTube-VIS, 180 on OVIS): 2.5-3x faster than the tile kernels
    ("A", 1, 60, torch.float32, "tile kernel, several waves per tile", "one source frame per workgroup"),
    ("S", 1, 180, torch.float16, "tile kernel, several waves per tile", "one source frame per workgroup"),
    # the bench batch
    ("A", 16, 300, torch.float32, "resident-slab kernel, 1 tiles per wave", "one source frame per workgroup"),
    ("A", 16, 300, torch.bfloat16, "resident-slab kernel, 4 tiles per wave", "one source frame per workgroup"),
    # large maps outside the slab: no frame split (12-20 % slower there)
    ("B", 16, 300, torch.float32, "resident-slab kernel, 1 tiles per wave", "resident-slab kernel, grad_loc/grad_attn)"),
    ("S", 16, 300, torch.float32, "resident-slab kernel, 1 tiles per wave", "resident-slab kernel, grad_loc/grad_attn)"),
    ("S", 16, 300, torch.bfloat16, "resident-slab kernel", "one source frame per workgroup"),
    # encoder-shaped calls: slab kernels while three levels fit, window kernels when a 4-byte slab holds two or fewer
    ("A", 1, None, torch.float32, "resident-slab kernel, 2 tiles per wave", "resident-slab kernel, grad_loc/grad_attn)"),
    ("A", 1, None, torch.bfloat16, "resident-slab kernel, 4 tiles per wave", "resident-slab kernel, grad_loc/grad_attn)"),
    ("S", 1, None, torch.float32, "resident-window kernel", "resident-window kernel"),
    ("S", 1, None, torch.bfloat16, "resident-slab kernel, 2 tiles per wave", "resident-slab kernel, grad_loc/grad_attn)"),
    # four clips in fp32: one round of (clip, head, part) workgroups -> the frame-split grid; not in 2-byte types
    ("A", 4, 300, torch.float32, "resident-slab kernel, 1 tiles per wave", "one source frame per workgroup"),
    ("A", 4, 300, torch.bfloat16, "resident-slab kernel, 1 tiles per wave", "resident-slab kernel, grad_loc/grad_attn)"),
]

# Single-frame decoder-like forwards: (pyramid, images, queries, dtype, forward label).  36 images x 300 queries on the SwinL pyramid
# in fp32: the slab would start at level 2 and 19 tiles would sit on 2 x 16 waves -- the tile forward is 30 % faster there; on the
# 360x640 pyramid the slab kernel stays.
SINGLE_FRAME_FORWARD_ROUTES = [
    ("S", 36, 300, torch.float32, "tile kernel"),
    ("A", 36, 300, torch.float32, "resident-slab kernel"),
]

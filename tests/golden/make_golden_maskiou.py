"""Records tests/golden/maskiou_*.npz from the REFERENCE's clip stitching, in float64 on the CPU: Tracker.process_masks
(src/models/tracker.py) makes the full-resolution probability maps and, through encode_mask, the maps > 0.5;
HungarianInferenceMatcher.compute_volumetric_iou_cost and compute_frame_average_iou_cost (src/models/matcher.py; both call
soft_iou) make the two cost matrices from the reference's own Track objects.  Tensors only; a few kilobytes each.

    python tests/golden/make_golden_maskiou.py [/path/to/reference]

The reference modules are imported as make_golden_attmap.py imports the segmentation module: a package whose __init__ is
skipped, with pycocotools, cv2, matplotlib and the util modules as stand-ins.  The stand-in of pycocotools' ``encode`` hands
back the array it was given, which is how the thresholded map is recorded.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

from maskiou_oracle import blob_logits  # noqa: E402


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a placeholder class (enough for `from x import Y`)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference():
    src = os.path.join(REFERENCE, "src")
    top = types.ModuleType("refsrc"); top.__path__ = [src]; sys.modules["refsrc"] = top
    pkg = types.ModuleType("refsrc.models"); pkg.__path__ = [os.path.join(src, "models")]; sys.modules["refsrc.models"] = pkg
    names = ["pycocotools", "cv2", "matplotlib", "matplotlib.pyplot", "refsrc.util", "refsrc.util.misc",
             "refsrc.util.viz_utils", "refsrc.util.box_ops", "refsrc.util.mask_ops"]
    try:
        import scipy.optimize  # noqa: F401
    except ImportError:
        names += ["scipy", "scipy.optimize"]
    for name in names:
        sys.modules.setdefault(name, _Anything(name))
    coco = types.ModuleType("pycocotools.mask")
    coco.encode = lambda bits: {"counts": b"", "bits": np.array(bits)}
    sys.modules["pycocotools.mask"] = coco
    sys.modules["pycocotools"].mask = coco
    return importlib.import_module("refsrc.models.tracker"), importlib.import_module("refsrc.models.matcher")


CASES = {   # name -> (Na, Nb, F, (h, w), (H, W))
    "maskiou_up": (4, 5, 1, (7, 9), (27, 35)),
    "maskiou_video": (3, 3, 2, (12, 20), (45, 80)),
    "maskiou_down": (2, 3, 1, (26, 22), (13, 11)),
}


def make_logits(seed, Na, Nb, F, h, w):
    """Blob fields; b[0] is a[0] (an identical pair), and a[1] / b[1] are far from zero with their positive regions in
    opposite corners (a disjoint pair)."""
    a, b = blob_logits(Na, F, h, w, seed), blob_logits(Nb, F, h, w, seed + 1)
    b[0] = a[0]
    a[1], b[1] = -8.0, -8.0
    a[1, :, : h // 3, : w // 3] = 8.0
    b[1, :, h - h // 3:, w - w // 3:] = 8.0
    return a, b


def main():
    tracker_mod, matcher_mod = import_reference()
    for seed, (name, (Na, Nb, F, (h, w), size)) in enumerate(sorted(CASES.items())):
        a, b = make_logits(2000 + 10 * seed, Na, Nb, F, h, w)
        tracker = object.__new__(tracker_mod.Tracker)
        tracker.overlap_window = F
        costs, bits = {}, {}
        for mode in ("volume", "frame"):
            matcher = matcher_mod.HungarianInferenceMatcher(overlap_window=F, use_frame_average_iou=mode == "frame")
            tracker.hungarian_matcher = matcher
            tracks = []
            for side, maps in (("a", a), ("b", b)):
                row = []
                for n in range(maps.shape[0]):
                    # the first clip, every frame inside the overlap window: every frame is kept as a probability map
                    kept = tracker.process_masks(0, 0, size, maps[n])
                    assert len(kept) == F and all(torch.is_tensor(m) and tuple(m.shape) == size for m in kept)
                    track = tracker_mod.Track(n, F, 0)
                    track.masks, track.mask_id, track.last_t = kept, "%s%d" % (side, n), F
                    row.append(track)
                tracks.append(row)
            fn = matcher.compute_frame_average_iou_cost if mode == "frame" else matcher.compute_volumetric_iou_cost
            costs[mode] = fn(tracks[0], tracks[1])
            assert costs[mode].shape == (Na, Nb) and costs[mode].dtype == np.float64
        # the thresholded maps, through the reference's encode_mask (binary mask IoU: every frame is encoded at once)
        tracker.hungarian_matcher = matcher_mod.HungarianInferenceMatcher(overlap_window=F, use_binary_mask_iou=True)
        for side, maps in (("a", a), ("b", b)):
            rows = [[rle["bits"] for rle in tracker.process_masks(0, 0, size, maps[n])] for n in range(maps.shape[0])]
            bits[side] = np.array(rows)
            assert bits[side].dtype == np.bool_ and bits[side].shape == (maps.shape[0], F) + size
        d = {"a": a.numpy(), "b": b.numpy(), "size": np.array(size, dtype=np.int64), "iou_volume": costs["volume"],
             "iou_frame": costs["frame"], "bits_a": bits["a"], "bits_b": bits["b"]}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
        print("wrote %s: volume iou %.4f .. %.4f, identical %.4f, disjoint %.2e" % (
            name, costs["volume"].min(), costs["volume"].max(), costs["volume"][0, 0], costs["volume"][1, 1]))


if __name__ == "__main__":
    main()

"""Drop-ins for the clip stitching of the reference's tracker (``src/models/tracker.py``, ``src/models/matcher.py``) on the
operators of include/maskiou.h (wired by :func:`devis_amd.patch_tracker`).

The reference resamples every trajectory's logit map to the video's resolution, one map at a time, keeps the float
probability maps of the stitching frames on the GPU, copies float maps to the host to threshold them there, and computes the
stitching cost pair by pair with a host synchronisation each.  Here a track keeps the small logit map (:class:`LogitMask`),
the maps to encode are binarised by one kernel call into bytes in the encoder's own memory order, and the cost matrix is one
operator call and one host copy.  With ``patch_tracker(..., gpu_rle=True)`` the maps to encode never become bytes: the device
counts their run lengths (include/maskrle.h) and the host packs the counts (:func:`encode_logits_rle`).  With
``patch_tracker(..., gpu_binary_iou=True)`` the reference's other cost, the IoU of the binarised masks
(``use_binary_mask_iou``), takes the same route: the stitching frames stay logit maps and the cost matrix is one
:func:`devis_amd.mask_binary_iou` call (include/maskbiou.h) in place of a host loop over pairs of
encodings.
"""
import numpy as np
import torch


class LogitMask:
    """A mask a track keeps for clip stitching: the mask head's ``[h, w]`` logit map and the size it stands for, in place of
    the full-resolution probability map.  Neither a ``dict`` (an encoded mask) nor ``None`` (no detection), so the
    reference's checks of ``Track.masks`` treat it as they treat a tensor."""

    __slots__ = ("logits", "size")

    def __init__(self, logits, size):
        if logits.dim() != 2:
            raise ValueError("LogitMask: logits must be [h, w], got %s" % (tuple(logits.shape),))
        self.logits = logits.detach()
        self.size = (int(size[0]), int(size[1]))

    def probabilities(self):
        """The map the reference keeps: ``[H, W]`` probabilities, by torch."""
        x = torch.nn.functional.interpolate(self.logits[None, None], self.size, mode="bilinear", align_corners=False)
        return x.sigmoid()[0, 0]

    def __repr__(self):
        return "LogitMask(%s -> %s, %s)" % (tuple(self.logits.shape), self.size, self.logits.dtype)


def encode_logits(logits, size, mask_util):
    """The run-length encodings of ``logits`` [N, h, w] at ``size``, as the reference's ``encode_mask`` returns them: one
    :func:`devis_amd.binarize_masks` call in Fortran order, one host copy of bytes, then ``mask_util.encode`` per mask."""
    from .ops import binarize_masks
    with torch.no_grad():
        bits = binarize_masks(logits, size, order="F")
    host = bits.transpose(1, 2).cpu().numpy()           # the dense [N, W, H] buffer
    out = []
    for n in range(host.shape[0]):
        rle = mask_util.encode(host[n].T)               # [H, W], Fortran-contiguous, no copy
        rle["counts"] = rle["counts"].decode("utf-8")
        out.append(rle)
    return out


def encode_logits_rle(logits, size, mask_util, max_runs=None):
    """:func:`encode_logits` without the byte map: one :func:`devis_amd.mask_run_lengths` call, one host copy of the rows (a
    few KB per mask), then ``mask_util.frPyObjects`` on each mask's counts -- the encoder's string packer on an uncompressed
    encoding.  A mask with more runs than the cap (``max_runs``; the operator's default when None) is never encoded from its
    truncated row: those masks go through :func:`encode_logits` together, and the results come back in the order of
    ``logits``."""
    from .ops import mask_run_lengths
    H, W = int(size[0]), int(size[1])
    with torch.no_grad():
        runs = mask_run_lengths(logits, (H, W), max_runs=max_runs)
    host = runs.cpu().numpy()
    cap = host.shape[1] - 1
    out, over = [None] * host.shape[0], []
    for n in range(host.shape[0]):
        count = int(host[n, 0])
        if count > cap:
            over.append(n)
            continue
        rle = mask_util.frPyObjects({"size": [H, W], "counts": host[n, 1:1 + count].tolist()}, H, W)
        rle["counts"] = rle["counts"].decode("utf-8")
        out[n] = rle
    if over:
        for n, rle in zip(over, encode_logits(logits[over], (H, W), mask_util)):
            out[n] = rle
    return out


def frames_to_encode(use_binary_mask_iou, overlap_window, start_idx, idx, num_masks):
    """Which of a clip's ``num_masks`` frames the reference's ``process_masks`` encodes at once (the others are kept for
    stitching): all of them for binary mask IoU; else, for the first clip, those before the last ``overlap_window`` frames,
    and for a later clip those between the two overlaps and those before ``start_idx``."""
    if use_binary_mask_iou:
        return [True] * num_masks
    if idx == 0:
        return [t < num_masks - overlap_window for t in range(num_masks)]
    return [overlap_window + start_idx <= t < num_masks - overlap_window or t < start_idx for t in range(num_masks)]


def _encoder(gpu_rle):
    return encode_logits_rle if gpu_rle else encode_logits


def make_process_masks(tracker_module, gpu_rle=False, gpu_binary_iou=False):
    encode_frames = _encoder(gpu_rle)

    def process_masks(self, start_idx, idx, tgt_size, masks):
        """Drop-in for ``Tracker.process_masks``: the reference's choice of frames; the frames to encode through one
        binarise call (one run-length call with ``gpu_rle``), the kept ones as :class:`LogitMask`.  With ``gpu_binary_iou``
        binary mask IoU keeps the stitching frames too, as the soft cost does; the track's own schedule encodes each as it
        leaves the window."""
        num_masks = masks.shape[0]
        binary = self.hungarian_matcher.use_binary_mask_iou and not gpu_binary_iou
        encode = frames_to_encode(binary, self.overlap_window, start_idx, idx, num_masks)
        which = [t for t in range(num_masks) if encode[t]]
        processed = [None if encode[t] else LogitMask(masks[t], tgt_size) for t in range(num_masks)]
        if which:
            picked = masks.detach() if len(which) == num_masks else masks.detach()[which]
            for t, rle in zip(which, encode_frames(picked, tgt_size, tracker_module.mask_util)):
                processed[t] = rle
        return processed

    return process_masks


def make_encode_mask(tracker_module, previous, gpu_rle=False):
    encode_frames = _encoder(gpu_rle)

    def encode_mask(mask):
        """Drop-in for the tracker module's ``encode_mask``: a :class:`LogitMask` is binarised on the GPU; anything else
        goes to the replaced function."""
        if isinstance(mask, LogitMask):
            return encode_frames(mask.logits[None], mask.size, tracker_module.mask_util)[0]
        return previous(mask)

    return encode_mask


def _stack(masks_per_track):
    """[N, F, h, w] logits and the common target size of the tracks' LogitMasks."""
    size, rows = None, []
    for masks in masks_per_track:
        for m in masks:
            if not isinstance(m, LogitMask):
                raise TypeError("expected a LogitMask among the stitching frames' masks, got %s" % type(m).__name__)
            if size is None:
                size = m.size
            elif m.size != size:
                raise RuntimeError("the stitching frames' masks stand for different sizes: %s and %s" % (size, m.size))
        rows.append(torch.stack([m.logits for m in masks]))
    return torch.stack(rows), size


def _stack_binary(masks_per_track):
    """:func:`_stack` for the binary cost, where a frame without a detection (None) counts as an empty mask: None when the
    windows hold no LogitMask at all (encodings and None only), else ([N, F, h, w] logits, the common target size) with a map
    of zeros -- no pixel set -- for every None.  Encodings beside LogitMasks raise TypeError."""
    first, encoded = None, False
    for masks in masks_per_track:
        for m in masks:
            if isinstance(m, LogitMask):
                first = first or m
            elif m is not None:
                if not isinstance(m, dict):
                    raise TypeError("expected a LogitMask, an encoded mask or None among the stitching frames' masks, got %s"
                                    % type(m).__name__)
                encoded = True
    if first is None:
        return None
    if encoded:
        raise TypeError("the stitching frames hold encoded masks beside LogitMasks: the binary mask IoU takes a window of "
                        "one kind")
    empty = LogitMask(torch.zeros_like(first.logits), first.size)
    return _stack([[empty if m is None else m for m in masks] for masks in masks_per_track])


def _binary_iou_cost(matcher, previous, track1, track2, reduce):
    """The binary cost of :func:`make_iou_cost`: the windows' maps stacked, one :func:`devis_amd.mask_binary_iou` call, one
    host copy.  A window without a LogitMask goes to the replaced method."""
    if not len(track1) or not len(track2):
        return np.zeros([len(track1), len(track2)])
    windows1 = [track.get_last_results(matcher.overlap_w, "masks") for track in track1]
    windows2 = [track.get_first_results(matcher.overlap_w, "masks") for track in track2]
    both = _stack_binary(windows1 + windows2)
    if both is None:
        return previous(matcher, track1, track2)
    maps, size = both
    from .ops import mask_binary_iou
    with torch.no_grad():
        iou = mask_binary_iou(maps[:len(track1)], maps[len(track1):], size, reduce=reduce)
    return iou.cpu().numpy()


def make_get_formatted_result(previous):
    def get_formatted_result(self, *args, **kwargs):
        """Drop-in for ``Track.get_formatted_result`` beside ``gpu_binary_iou``: the reference skips its final
        ``encode_all_masks()`` in binary mode, where its masks are encodings from the start; here the last clip's trailing
        window still holds :class:`LogitMask` s, which are encoded first."""
        self.encode_all_masks()
        return previous(self, *args, **kwargs)

    return get_formatted_result


def make_iou_cost(previous, reduce, gpu_binary_iou=False):
    def iou_cost(self, track1, track2):
        """Drop-in for ``HungarianInferenceMatcher.compute_volumetric_iou_cost`` / ``compute_frame_average_iou_cost`` for
        soft IoU: the tracks' logit maps stacked, one :func:`devis_amd.mask_soft_iou` call, one host copy; float64
        ``[len(track1), len(track2)]`` as the reference returns.  (Every pair is computed: the reference's reuse of a value
        for equal mask ids gives the same numbers.)  With ``use_binary_mask_iou`` the replaced method runs, or -- with
        ``gpu_binary_iou`` -- one :func:`devis_amd.mask_binary_iou` call on the same stacked maps, a frame without a
        detection as an empty mask (the reference's ``iou`` adds the other mask's area to the union and nothing to the
        intersection: what an empty mask gives)."""
        if self.use_binary_mask_iou:
            if gpu_binary_iou:
                return _binary_iou_cost(self, previous, track1, track2, reduce)
            return previous(self, track1, track2)
        if not len(track1) or not len(track2):
            return np.zeros([len(track1), len(track2)])
        from .ops import mask_soft_iou
        a, size = _stack([track.get_last_results(self.overlap_w, "masks") for track in track1])
        b, size_b = _stack([track.get_first_results(self.overlap_w, "masks") for track in track2])
        if size_b != size:
            raise RuntimeError("the stitching frames' masks stand for different sizes: %s and %s" % (size, size_b))
        with torch.no_grad():
            iou = mask_soft_iou(a, b, size, reduce=reduce)
        return iou.cpu().numpy().astype(np.float64)

    return iou_cost

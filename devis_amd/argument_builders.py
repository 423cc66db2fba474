"""Cached form of the one call-site argument builder the reference exposes as a function:
``DeformableTransformerEncoder.get_reference_points`` (``src/models/deformable_transformer.py:185-198``), which the
DeVIS encoder stack calls once per forward (``devis_transformer.py:95``).  The reference rebuilds two ``linspace`` s and
a ``meshgrid`` per pyramid level per call -- each ``linspace`` reads its bounds from the device tensor
``spatial_shapes``, i.e. synchronises -- although the centre grids only depend on the pyramid.  Here the grids are
cached per pyramid (read from the host copy ``_native.shapes_hint`` already keeps per ``spatial_shapes`` tensor), and
only the per-call arithmetic with ``valid_ratios`` runs, in the reference's order: the result is bit-identical
(``tests/test_host_cpu.py::test_cached_reference_points_match_the_reference_call_site``, fixture made by the
reference).

``DeformableTransformer.prepare_data`` (``deformable_transformer.py:69-94``) is the other one: it has every ``(h, w)`` as Python
ints (``:74-75``), pushes them to the device as a NEW ``spatial_shapes`` tensor each forward (``:87``: a blocking copy) and derives
``level_start_index`` from it on the device.  ``patch_transformer`` replaces it by :func:`prepare_data`, which does the same
flattening and takes the two tensors from :func:`interned_pyramid` -- one device pair per pyramid and device, built from the
same Python ints and registered with the binding together with their host values (``_native.register_host_values``) -- so that
the operator's kernel selection never reads the device, and a ``devis_amd.graphed`` layer sees the same pyramid (by value) step
after step: one capture, no synchronisation.

Opt-in wiring, no DeVIS source change::

    import src.models.deformable_transformer as dt, src.models.devis_transformer as dvt
    devis_amd.patch_transformer(dt, dvt)

The other call-site tensors (temporal offsets, repeated shapes: ``devis_transformer.py:97-118,146-158``) are built inline in the
reference's ``forward`` s from the frame count alone.  With the second argument each frame's offsets tensor is interned as well
(:class:`_InterningTorch`); without it the attention modules consume new ones as they come
(``TemporalMSDeformAttnBase._frame_table``: one cached, synchronisation-free device table per list of offsets), and a
``devis_amd.graphed`` layer copies them into its captured arguments before each replay (a few bytes, device to device).
"""

import torch

_grid_cache = {}
_captured = {}
_MAX_ENTRIES = 32


def _pyramid(spatial_shapes):
    """[(H, W), ...] as Python ints.  A device tensor is read through the per-tensor host copy the operator keeps
    anyway (one device-to-host copy per distinct tensor)."""
    if isinstance(spatial_shapes, torch.Tensor):
        if spatial_shapes.is_cuda:
            from . import _native
            hint = _native.shapes_hint(spatial_shapes)
            if hint is None:
                raise RuntimeError("get_reference_points: spatial_shapes is a device tensor first seen inside a HIP-graph capture; "
                                   "call once outside the capture (or pass the sizes as Python ints)")
            flat = list(hint)
        else:
            flat = spatial_shapes.reshape(-1).tolist()
        return tuple((int(flat[2 * i]), int(flat[2 * i + 1])) for i in range(len(flat) // 2))
    return tuple((int(h), int(w)) for h, w in spatial_shapes)


def get_reference_points(spatial_shapes, valid_ratios, device):
    """Drop-in for the reference's static method (same arguments, same result, ``[N, S, L, 2]``): pixel centres of
    every level, normalised by the valid part of the (padded) frame."""
    shapes = _pyramid(spatial_shapes)
    key = (shapes, str(device))
    capturing = torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()
    grids = _grid_cache.get(key)
    if grids is not None and capturing:
        _captured[id(grids)] = grids            # a HIP graph now holds these addresses: out of the cache's reach for good (keyed by
                                                # the grid set itself: after an eviction one key may have had several live sets)
    if grids is None:
        grids = []
        for H_, W_ in shapes:
            ref_y, ref_x = torch.meshgrid(torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device),
                                          torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device),
                                          indexing='ij')
            grids.append((ref_y.reshape(-1)[None], ref_x.reshape(-1)[None]))
        if not capturing:                       # (grids built INSIDE a capture live in the graph's memory pool: never shared)
            if len(_grid_cache) >= _MAX_ENTRIES:
                _grid_cache.clear()
            _grid_cache[key] = grids
    per_level = []
    for lvl, ((H_, W_), (gy, gx)) in enumerate(zip(shapes, grids)):
        ref_y = gy / (valid_ratios[:, None, lvl, 1] * H_)
        ref_x = gx / (valid_ratios[:, None, lvl, 0] * W_)
        per_level.append(torch.stack((ref_x, ref_y), -1))
    points = torch.cat(per_level, 1)
    return points[:, :, None] * valid_ratios[:, None]


_pyramids = {}          # (shapes, device) -> (spatial_shapes, level_start_index): interned for good (a few hundred bytes per pyramid)


def interned_pyramid(shapes, device):
    """The device tensors ``(spatial_shapes [L, 2], level_start_index [L])`` (int64, as ``prepare_data`` builds them:
    deformable_transformer.py:87-91) of a pyramid given as Python ints -- ONE pair per (pyramid, device), built without reading
    the device and registered with the binding together with their host values."""
    shapes = tuple((int(h), int(w)) for h, w in shapes)
    device = torch.device(device)
    key = (shapes, str(device))
    hit = _pyramids.get(key)
    if hit is None:
        from . import _native
        starts, acc = [], 0
        for h, w in shapes:
            starts.append(acc)
            acc += h * w
        spatial = torch.as_tensor(shapes, dtype=torch.long, device=device)
        level_start = torch.as_tensor(starts, dtype=torch.long, device=device)
        if device.type == "cuda":
            _native.register_host_values(spatial, [v for hw in shapes for v in hw])
            _native.register_host_values(level_start, starts)
        hit = _pyramids[key] = (spatial, level_start)
    return hit


def flatten_sources(srcs):
    """``src_flatten`` of both ``prepare_data`` variants: ``cat([src.flatten(2).transpose(1, 2) for src in srcs], 1)``.  With plain
    tensors exactly that, bit for bit; when every level is a :class:`devis_amd.DeferredInputProjection`
    (:func:`patch_input_proj`) of one ``N``, ``C``, ``num_groups``, ``eps`` and dtype, ONE :func:`devis_amd.group_norm_tokens`
    call, each level then bound to its ``[N, C, H, W]`` view of the result; a mix materialises the deferred ones first."""
    from .modules import input_projection
    return input_projection.flatten_sources(list(srcs))


def prepare_data(self, srcs, masks, pos_embeds):
    """Replacement for ``DeformableTransformer.prepare_data`` (deformable_transformer.py:69-94; same arguments, same six results):
    per level the feature map, its padding mask and its positional embedding (+ the level embedding) flattened and concatenated
    over the levels, the valid ratios of every frame -- and the pyramid's ``spatial_shapes`` / ``level_start_index`` taken from
    :func:`interned_pyramid` instead of being pushed to the device again (the reference's ``torch.as_tensor(..., device=...)`` of a
    Python list is a blocking host-to-device copy: it waits for everything queued on the stream)."""
    pads, embeds = [], []
    for lvl, (mask, pos_embed) in enumerate(zip(masks, pos_embeds)):
        pads.append(mask.flatten(1))
        embeds.append(pos_embed.flatten(2).transpose(1, 2) + self.level_embed[lvl].view(1, 1, -1))
    src_flatten, mask_flatten, lvl_pos_embed_flatten = flatten_sources(srcs), torch.cat(pads, 1), torch.cat(embeds, 1)
    spatial_shapes, level_start_index = interned_pyramid([src.shape[-2:] for src in srcs], src_flatten.device)
    valid_ratios = torch.stack([self.get_valid_ratio(m) for m in masks], 1)
    return src_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index, valid_ratios


_int_tensors = {}       # (values, dtype, device) -> tensor: interned for good (tens of bytes each)


class _InterningTorch:
    """Stands in for the name ``torch`` INSIDE ``src.models.devis_transformer`` (only there): every attribute is torch's own, except
    that ``torch.tensor(<short list of Python ints>, device=<device>)`` -- how the stacks build each frame's ``temporal_offsets`` on
    every forward (devis_transformer.py:100, 113, 149) -- returns one interned device tensor per (values, device) instead of a new
    blocking host-to-device copy.  The tensors are read-only by convention (the stacks only index with them)."""

    def __init__(self, real):
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def tensor(self, data, *args, **kwargs):
        if (not args and isinstance(data, (list, tuple)) and 0 < len(data) <= 256 and all(type(v) is int for v in data) and
                kwargs.get("device") is not None and set(kwargs) <= {"device", "dtype"}):
            device = self._real.device(kwargs["device"])
            key = (tuple(data), kwargs.get("dtype"), str(device))
            hit = _int_tensors.get(key)
            if hit is None:
                hit = _int_tensors[key] = self._real.tensor(data, dtype=kwargs.get("dtype"), device=device)
                if device.type == "cuda":
                    from . import _native
                    _native.register_host_values(hit, data)
            return hit
        return self._real.tensor(data, *args, **kwargs)


def patch_transformer(deformable_transformer_module, devis_transformer_module=None):
    """Opt-in: make the reference's encoder stacks (``DeformableTransformerEncoder`` and its subclass
    ``DeVISTransformerEncoder``) use the cached :func:`get_reference_points`, and ``DeformableTransformer.prepare_data`` (inherited
    by ``DeVISTransformer``) the interning :func:`prepare_data`.  Pass the imported reference module
    ``src.models.deformable_transformer``; with ``src.models.devis_transformer`` as the second argument the temporal offsets its
    stacks build on every forward are interned too (:class:`_InterningTorch`), which takes the last blocking copies out of a
    training step.  Returns the replaced ``get_reference_points`` (to undo the first patch; :func:`unpatch_transformer` undoes
    all of them)."""
    cls = deformable_transformer_module.DeformableTransformerEncoder
    previous = cls.__dict__.get("get_reference_points")
    cls.get_reference_points = staticmethod(get_reference_points)
    top = getattr(deformable_transformer_module, "DeformableTransformer", None)
    if top is not None and "prepare_data" in top.__dict__ and top.__dict__["prepare_data"] is not prepare_data:
        top._devis_amd_prepare_data = top.__dict__["prepare_data"]
        top.prepare_data = prepare_data
    if devis_transformer_module is not None and not isinstance(getattr(devis_transformer_module, "torch", None), _InterningTorch):
        devis_transformer_module.torch = _InterningTorch(devis_transformer_module.torch)
    return previous


def unpatch_transformer(deformable_transformer_module, previous_get_reference_points, devis_transformer_module=None):
    """Undo :func:`patch_transformer` (tests)."""
    deformable_transformer_module.DeformableTransformerEncoder.get_reference_points = previous_get_reference_points
    top = getattr(deformable_transformer_module, "DeformableTransformer", None)
    if top is not None and "_devis_amd_prepare_data" in top.__dict__:
        top.prepare_data = top.__dict__["_devis_amd_prepare_data"]
        del top._devis_amd_prepare_data
    if devis_transformer_module is not None and isinstance(getattr(devis_transformer_module, "torch", None), _InterningTorch):
        devis_transformer_module.torch = devis_transformer_module.torch._real


def patch_mask_head(deformable_segmentation_module):
    """Opt-in: make the reference's mask head (``src.models.deformable_segmentation``) build its convolutions from
    :class:`devis_amd.modules.ModulatedDeformableConv2d` -- the HIP operator instead of ``torchvision.ops.deform_conv2d``.  Call
    it before the model is built: the mask head looks the class up by name when it is constructed; layers that already
    exist keep their class.  State dicts are interchangeable (same parameter names).  Returns the replaced class (to undo
    the patch; :func:`unpatch_mask_head`)."""
    from .modules import ModulatedDeformableConv2d
    previous = getattr(deformable_segmentation_module, "ModulatedDeformableConv2d")
    deformable_segmentation_module.ModulatedDeformableConv2d = ModulatedDeformableConv2d
    return previous


def unpatch_mask_head(deformable_segmentation_module, previous_class):
    """Undo :func:`patch_mask_head` (tests)."""
    deformable_segmentation_module.ModulatedDeformableConv2d = previous_class


def patch_attention_maps(deformable_segmentation_module):
    """Opt-in: make the reference's segmentation models (``src.models.deformable_segmentation``) build their
    ``bbox_attention`` from :class:`devis_amd.modules.MultiScaleMHAttentionMap` -- the fused HIP operator instead of
    einsum, masked_fill and softmax.  Call it before the model is built: the class is looked up by name at construction.
    State dicts are interchangeable (same parameter names).  Returns the replaced class (to undo the patch;
    :func:`unpatch_attention_maps`).  :func:`patch_mask_head` is a separate choice."""
    from .modules import MultiScaleMHAttentionMap
    previous = getattr(deformable_segmentation_module, "MultiScaleMHAttentionMap")
    deformable_segmentation_module.MultiScaleMHAttentionMap = MultiScaleMHAttentionMap
    return previous


def unpatch_attention_maps(deformable_segmentation_module, previous_class):
    """Undo :func:`patch_attention_maps` (tests)."""
    deformable_segmentation_module.MultiScaleMHAttentionMap = previous_class


def patch_mask_head_stages(deformable_segmentation_module):
    """Opt-in: make the reference's segmentation models (``src.models.deformable_segmentation``) build their ``mask_head``
    from :class:`devis_amd.modules.MaskHeadConv` -- GroupNorm, ReLU, upsampling, the FPN add and the concatenation of the
    attention maps as one fused HIP operator per stage, and the deformable convolutions as
    :class:`devis_amd.modules.ModulatedDeformableConv2d`.  Call it before the model is built: the class is looked up by
    name at construction.  State dicts are interchangeable (same parameter names).  Returns the replaced class (to undo the
    patch; :func:`unpatch_mask_head_stages`).  :func:`patch_mask_head` and :func:`patch_attention_maps` are separate
    choices."""
    from .modules import MaskHeadConv
    previous = getattr(deformable_segmentation_module, "MaskHeadConv")
    deformable_segmentation_module.MaskHeadConv = MaskHeadConv
    return previous


def unpatch_mask_head_stages(deformable_segmentation_module, previous_class):
    """Undo :func:`patch_mask_head_stages` (tests)."""
    deformable_segmentation_module.MaskHeadConv = previous_class


def pad_masks(masks):
    """The targets' mask stacks ``[n_i, H_i, W_i]`` as one zero-padded ``[B, max n, max H, max W]`` tensor in their own
    dtype (bool stays bool): what the reference's nested tensor holds, without its padding mask."""
    size = [max(m.shape[d] for m in masks) for d in range(3)]
    out = masks[0].new_zeros([len(masks)] + size)
    for slot, m in zip(out, masks):
        slot[:m.shape[0], :m.shape[1], :m.shape[2]].copy_(m)
    return out


def loss_masks(self, outputs, targets, indices, num_boxes):
    """A drop-in for the reference's ``SetCriterion.loss_masks`` (``self`` is the criterion) on :func:`devis_amd.mask_losses`:
    the same choice of target masks -- image matchings ``(src, tgt)`` and DeVIS's ``(src, tgt, mask)`` ones, whose
    predictions are filtered by the first clip's mask when that mask selects nothing -- and the same padding of the targets
    to the largest size, but the bool targets stay bool and the logits stay small: resampling, focal loss and dice loss are
    one operator.  Returns ``{"loss_mask", "loss_dice"}``."""
    from .ops import mask_losses
    assert "pred_masks" in outputs
    src_masks = outputs["pred_masks"]
    if len(indices[0]) == 3:
        keep = indices[0][2]
        if not torch.any(keep):
            tgt_idx = self._get_tgt_permutation_masked_idx(indices)
            src_masks = src_masks[keep]
        else:
            tgt_idx = self._get_tgt_permutation_idx(indices, True)
    else:
        tgt_idx = self._get_tgt_permutation_idx(indices)        # (the predictions are [N, 1, h, w] here: taken as they are)
    target_masks = pad_masks([t["masks"] for t in targets])[tgt_idx]
    return mask_losses(src_masks, target_masks, num_boxes)


def patch_mask_losses(criterion_module):
    """Opt-in: make the reference's criterion (``src.models.criterion``) compute its mask losses with :func:`loss_masks` --
    the fused HIP operator instead of interpolate, sigmoid_focal_loss and dice_loss.  Takes effect at once, also for
    criteria that already exist (the method is looked up on the class).  Returns the replaced function (to undo the patch;
    :func:`unpatch_mask_losses`).  The other patches are separate choices."""
    previous = criterion_module.SetCriterion.loss_masks
    criterion_module.SetCriterion.loss_masks = loss_masks
    return previous


def unpatch_mask_losses(criterion_module, previous):
    """Undo :func:`patch_mask_losses` (tests)."""
    criterion_module.SetCriterion.loss_masks = previous


def patch_tracker(tracker_module, matcher_module, *, gpu_rle=False, gpu_binary_iou=False):
    """Opt-in: make the reference's clip stitching (``src.models.tracker``, ``src.models.matcher``) run on
    :func:`devis_amd.binarize_masks` and :func:`devis_amd.mask_soft_iou` (:mod:`devis_amd.tracking`):
    ``Tracker.process_masks`` keeps the stitching frames as small :class:`devis_amd.LogitMask` s and encodes the others
    through one binarise call; the module's ``encode_mask`` accepts a ``LogitMask``; and
    ``HungarianInferenceMatcher.compute_volumetric_iou_cost`` / ``compute_frame_average_iou_cost`` compute the soft IoU
    matrix in one operator call (with ``use_binary_mask_iou`` they run as before, unless ``gpu_binary_iou`` is given).  Takes effect at once, also for trackers
    and matchers that already exist.  Returns what was replaced (to undo the patch; :func:`unpatch_tracker`).  The other
    patches are separate choices.

    ``gpu_rle=True`` (an opt-in of its own): the frames to encode go through :func:`devis_amd.mask_run_lengths` and the
    module's ``mask_util.frPyObjects`` instead of the byte map and ``mask_util.encode``
    (:func:`devis_amd.tracking.encode_logits_rle`); a mask with more runs than the operator's cap still takes the byte path.
    Raises AttributeError, before anything is replaced, when the module's ``mask_util`` has no ``frPyObjects``.

    ``gpu_binary_iou=True`` (an opt-in of its own, which combines freely with ``gpu_rle``): a matcher whose
    ``use_binary_mask_iou`` is true takes the same route as the soft cost -- ``process_masks`` keeps the stitching frames
    as ``LogitMask`` s, which the track's own schedule encodes as they leave the window, and the two cost methods make one
    :func:`devis_amd.mask_binary_iou` call on the stacked maps (a frame without a detection counts as an empty mask; a
    window of encodings and None only goes to the replaced method).  The reference skips its final ``encode_all_masks()``
    in binary mode, so ``Track.get_formatted_result`` is wrapped to call it first; what it replaced is returned under a
    fifth key.  Raises AttributeError, before anything is replaced, when the tracker module has no ``Track``."""
    from . import tracking
    matcher = matcher_module.HungarianInferenceMatcher
    if gpu_binary_iou and not hasattr(tracker_module, "Track"):
        raise AttributeError("patch_tracker(gpu_binary_iou=True): the tracker module has no Track whose "
                             "get_formatted_result could encode the last stitching window")
    if gpu_rle and not hasattr(tracker_module.mask_util, "frPyObjects"):
        raise AttributeError("patch_tracker(gpu_rle=True): the tracker module's mask_util has no frPyObjects to pack the "
                             "run lengths with")
    previous = {"process_masks": tracker_module.Tracker.process_masks, "encode_mask": tracker_module.encode_mask,
                "compute_volumetric_iou_cost": matcher.compute_volumetric_iou_cost,
                "compute_frame_average_iou_cost": matcher.compute_frame_average_iou_cost}
    if gpu_binary_iou:
        previous["get_formatted_result"] = tracker_module.Track.get_formatted_result
        tracker_module.Track.get_formatted_result = tracking.make_get_formatted_result(previous["get_formatted_result"])
    tracker_module.Tracker.process_masks = tracking.make_process_masks(tracker_module, gpu_rle, gpu_binary_iou)
    tracker_module.encode_mask = tracking.make_encode_mask(tracker_module, previous["encode_mask"], gpu_rle)
    matcher.compute_volumetric_iou_cost = tracking.make_iou_cost(previous["compute_volumetric_iou_cost"], "volume", gpu_binary_iou)
    matcher.compute_frame_average_iou_cost = tracking.make_iou_cost(previous["compute_frame_average_iou_cost"], "frame", gpu_binary_iou)
    return previous


def unpatch_tracker(tracker_module, matcher_module, previous):
    """Undo :func:`patch_tracker` (tests)."""
    tracker_module.Tracker.process_masks = previous["process_masks"]
    tracker_module.encode_mask = previous["encode_mask"]
    matcher_module.HungarianInferenceMatcher.compute_volumetric_iou_cost = previous["compute_volumetric_iou_cost"]
    matcher_module.HungarianInferenceMatcher.compute_frame_average_iou_cost = previous["compute_frame_average_iou_cost"]
    if "get_formatted_result" in previous:          # (patched with gpu_binary_iou=True)
        tracker_module.Track.get_formatted_result = previous["get_formatted_result"]


# ---- the criterion: matching and box losses (include/boxmatch.h) ---------------------------------------------------------

def _solver():
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment


def _like_predictions(boxes, dtype):
    """Target boxes as :func:`devis_amd.match_cost` / :func:`devis_amd.box_losses` take them beside predictions of ``dtype``:
    as they are when they have that dtype (or float32 beside a 16-bit one), else converted."""
    if boxes.dtype == dtype or (boxes.dtype == torch.float32 and dtype in (torch.bfloat16, torch.float16)):
        return boxes
    return boxes.to(dtype)


def _costs_on_host(matcher, logits, boxes, tgt_labels, tgt_boxes, l1):
    """One :func:`devis_amd.match_cost` call and ONE device-to-host transfer that carries the cost and the status: the
    host's [L, R, T] cost.  Raises what the reference's indexing and asserts raise."""
    from . import ops
    cost, status = ops.match_cost(logits, boxes.to(logits.dtype), tgt_labels.long(), _like_predictions(tgt_boxes, logits.dtype),
                                  cost_class=matcher.cost_class, cost_bbox=matcher.cost_bbox, cost_giou=matcher.cost_giou,
                                  l1=l1, alpha=matcher.focal_alpha)
    packed = torch.cat([cost.reshape(-1), status.to(cost.dtype)]).cpu()        # the one synchronising transfer
    _raise_on_cost_counts(*(int(v) for v in packed[cost.numel():]), logits.shape[-1])
    return packed[:cost.numel()].reshape(cost.shape).numpy()


def _raise_on_cost_counts(bad_pred, bad_tgt, bad_label, num_classes=None):
    """What the reference's indexing and asserts raise, from the counts of :func:`devis_amd.match_cost`'s status."""
    if bad_label:
        raise IndexError("%d target label(s) outside %s" % (bad_label, "the classes" if num_classes is None else "[0, %d)" % num_classes))
    if bad_pred or bad_tgt:           # (the reference's asserts in multi_giou / generalized_box_iou)
        raise AssertionError("%d prediction and %d target box(es) with x1 < x0 or y1 < y0" % (bad_pred, bad_tgt))


def raise_on_match_status(status, num_classes=None):
    """The deferred check of a matching made without a transfer (``patch_criterion(gpu_assignment=True)``), and the one
    place that reads its status: ``status`` is ``matcher.last_match_status`` -- the three counts of
    :func:`devis_amd.match_cost` followed by the two of :func:`devis_amd.linear_assignment` -- or either operator's own
    status (told apart by their lengths 3 and 2), or None (a matching that launched nothing).  Synchronises.  Raises
    IndexError for labels outside the classes and AssertionError for degenerate boxes, as the host path of the patched
    matchers does, and ValueError with scipy's messages for a cost matrix with NaN or ``-inf`` entries and for an infeasible
    one.  ``num_classes`` only completes the IndexError's message."""
    if status is None:
        return
    counts = [int(v) for v in status.reshape(-1).tolist()]
    if len(counts) not in (2, 3, 5):
        raise ValueError("raise_on_match_status: a status of 5, 3 or 2 counts is expected, got %d" % len(counts))
    if len(counts) != 2:
        _raise_on_cost_counts(*counts[:3], num_classes)
    if len(counts) != 3:
        invalid, infeasible = counts[-2:]
        if invalid:
            raise ValueError("matrix contains invalid numeric entries (%d problem(s))" % invalid)
        if infeasible:
            raise ValueError("cost matrix is infeasible (%d problem(s))" % infeasible)


def _on_device_of(index, like):
    """A host index tensor on ``like``'s device without a synchronising copy."""
    if like.device.type == "cpu":
        return index
    return index.pin_memory().to(like.device, non_blocking=True)


def _devis_indices(matcher, dicts, targets):
    """``DeVISHungarianMatcher.forward`` for every dict of ``dicts`` (one cost call for all of them): per dict the
    reference's return value -- a list with the triple of batch element 0."""
    F, Q = matcher.num_frames, matcher.num_out
    first = dicts[0]["pred_logits"]
    if first.shape[0] == 0:                 # (the reference's loop does not run: it returns None)
        return [None] * len(dicts)
    tgt_ids, tgt_bbox, tgt_valid = targets[0]["labels"], targets[0]["boxes"], targets[0]["valid"]
    num_tgt = len(tgt_ids) // F
    frames = torch.arange(F)
    if num_tgt == 0:
        out = []
        for d in dicts:
            base = frames.long().to(d["pred_logits"].device)
            out.append([(base * Q, base, torch.zeros(F, device=d["pred_logits"].device, dtype=torch.bool))])
        return out
    C = first.shape[-1]
    if len(dicts) == 1:
        logits, boxes = first[0][None], dicts[0]["pred_boxes"][0][None]
    else:
        logits = torch.stack([d["pred_logits"][0] for d in dicts])
        boxes = torch.stack([d["pred_boxes"][0] for d in dicts])
    cost = _costs_on_host(matcher, logits.reshape(len(dicts), F, Q, C), boxes.reshape(len(dicts), F, Q, 4),
                          tgt_ids.reshape(num_tgt, F), tgt_bbox.reshape(num_tgt, F, 4),
                          "sum" if matcher.use_l1_distance_sum else "mean")
    valid = tgt_valid.reshape(num_tgt, F)
    solve, out = _solver(), []
    for c in cost:
        out_i, tgt_i = (torch.as_tensor(v, dtype=torch.int64) for v in solve(c))
        index_i = (frames[None] * Q + out_i[:, None]).reshape(-1)
        index_j = (frames[None] + tgt_i[:, None] * F).reshape(-1)
        index_valid = valid[_on_device_of(tgt_i, valid)].reshape(-1).type(torch.bool)
        out.append([(index_i, index_j, index_valid)])
    return out


def _devis_indices_on_device(matcher, dicts, targets):
    """:func:`_devis_indices` without a transfer (``patch_criterion(gpu_assignment=True)``): :func:`devis_amd.match_cost`,
    :func:`devis_amd.linear_assignment` on that cost as it lies, and the index arithmetic on the device, for all of
    ``dicts`` in one call each.  The triples have the reference's values and dtypes; ``index_i`` and ``index_j`` are on the
    predictions' device.  The five status counts are left, unread, as ``matcher.last_match_status``
    (:func:`raise_on_match_status`).  What the shapes put outside this route -- no batch element, a clip without targets, a
    problem beyond the operator's limits -- takes :func:`_devis_indices`."""
    from . import ops
    from .functions import assignment
    F, Q = matcher.num_frames, matcher.num_out
    first = dicts[0]["pred_logits"]
    tgt_ids, tgt_bbox, tgt_valid = targets[0]["labels"], targets[0]["boxes"], targets[0]["valid"]
    num_tgt = len(tgt_ids) // F
    if first.shape[0] == 0 or num_tgt == 0 or not assignment.fits(Q, num_tgt):
        matcher.last_match_status = None
        return _devis_indices(matcher, dicts, targets)
    L, C = len(dicts), first.shape[-1]
    if L == 1:
        logits, boxes = first[0][None], dicts[0]["pred_boxes"][0][None]
    else:
        logits = torch.stack([d["pred_logits"][0] for d in dicts])
        boxes = torch.stack([d["pred_boxes"][0] for d in dicts])
    logits = logits.reshape(L, F, Q, C)
    cost, cost_status = ops.match_cost(logits, boxes.reshape(L, F, Q, 4).to(logits.dtype), tgt_ids.reshape(num_tgt, F).long(),
                                       _like_predictions(tgt_bbox.reshape(num_tgt, F, 4), logits.dtype),
                                       cost_class=matcher.cost_class, cost_bbox=matcher.cost_bbox, cost_giou=matcher.cost_giou,
                                       l1="sum" if matcher.use_l1_distance_sum else "mean", alpha=matcher.focal_alpha)
    out_i, tgt_i, solve_status = ops.linear_assignment(cost)
    matcher.last_match_status = torch.cat([cost_status, solve_status])
    frames = torch.arange(F, device=out_i.device)
    index_i = (frames * Q + out_i[:, :, None]).reshape(L, -1)
    index_j = (frames + tgt_i[:, :, None] * F).reshape(L, -1)
    index_valid = tgt_valid.reshape(num_tgt, F)[tgt_i.to(tgt_valid.device)].reshape(L, -1).type(torch.bool)
    return [[(index_i[l], index_j[l], index_valid[l])] for l in range(L)]


def _image_indices(matcher, dicts, targets):
    """``HungarianMatcher.forward`` for every dict of ``dicts`` (one cost call for all of them)."""
    first = dicts[0]["pred_logits"]
    B, Q, C = first.shape
    if len(dicts) == 1:
        logits, boxes = first[None], dicts[0]["pred_boxes"][None]
    else:
        logits, boxes = torch.stack([d["pred_logits"] for d in dicts]), torch.stack([d["pred_boxes"] for d in dicts])
    tgt_ids = torch.cat([v["labels"] for v in targets])
    tgt_bbox = torch.cat([v["boxes"] for v in targets])
    cost = _costs_on_host(matcher, logits.reshape(len(dicts), 1, B * Q, C), boxes.reshape(len(dicts), 1, B * Q, 4),
                          tgt_ids.reshape(-1, 1), tgt_bbox.reshape(-1, 1, 4), "sum")
    sizes = [len(v["boxes"]) for v in targets]
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    solve, out = _solver(), []
    for c in cost:
        c = c.reshape(B, Q, c.shape[-1])
        pairs = [solve(c[i, :, s:s + n]) for i, (s, n) in enumerate(zip(starts, sizes))]
        out.append([(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in pairs])
    return out


def make_matcher_forward(previous, indices_of):
    """A ``forward`` of a matcher class on :func:`devis_amd.match_cost`; ``previous`` is what it replaces (and what runs with
    ``focal_loss=False``)."""
    @torch.no_grad()
    def forward(self, outputs, targets):
        if not self.focal_loss:
            return previous(self, outputs, targets)
        return indices_of(self, [outputs], targets)[0]
    forward.indices_of = indices_of
    return forward


def loss_boxes(self, outputs, targets, indices, num_boxes):
    """A drop-in for the reference's ``SetCriterion.loss_boxes`` (``self`` is the criterion) on :func:`devis_amd.box_losses`:
    the same choice of boxes -- image matchings ``(src, tgt)`` and DeVIS's ``(src, tgt, mask)`` ones, masked when the first
    clip's mask selects nothing -- then one operator call instead of ``l1_loss`` and the diagonal of an N x N GIoU matrix.
    The reference's two degenerate-box asserts (a synchronisation each) are not reproduced.  Returns
    ``{"loss_bbox", "loss_giou"}``."""
    from .ops import box_losses
    assert 'pred_boxes' in outputs
    if len(indices[0]) == 3:
        if not torch.any(indices[0][2]):
            target_boxes = torch.cat([t['boxes'][i[mask]] for t, (_, i, mask) in zip(targets, indices)], dim=0)
            idx = self._get_src_permutation_masked_idx(indices)
        else:
            target_boxes = torch.cat([t['boxes'][i] for t, (_, i, _) in zip(targets, indices)], dim=0)
            idx = self._get_src_permutation_idx(indices, True)
    else:
        target_boxes = torch.cat([t['boxes'][i] for t, (_, i) in zip(targets, indices)], dim=0)
        idx = self._get_src_permutation_idx(indices)
    src_boxes = outputs['pred_boxes'][idx]
    return box_losses(src_boxes, _like_predictions(target_boxes, src_boxes.dtype), num_boxes)


def make_criterion_forward(previous, matcher_forwards):
    """``SetCriterion.forward`` with the matchings of the top-level dict and of every aux dict made by ONE cost call, one
    transfer and one assignment per dict (``patch_criterion(batch_aux=True)``): the replaced ``forward`` gets shallow copies
    of the dicts that carry ``"indices"``, which it honours.  Anything the patched matchers do not cover passes straight
    through."""
    def forward(self, outputs, targets):
        patched = matcher_forwards.get(type(self.matcher))
        aux = outputs.get("aux_outputs", ())
        pending = [d for d in (outputs, *aux) if "indices" not in d]
        shapes = {(tuple(d["pred_logits"].shape), tuple(d["pred_boxes"].shape), d["pred_logits"].dtype) for d in pending}
        if (patched is None or type(self.matcher).forward is not patched or not self.matcher.focal_loss or len(pending) < 2
                or len(shapes) != 1):
            return previous(self, outputs, targets)
        with torch.no_grad():
            found = iter(patched.indices_of(self.matcher, [{k: v for k, v in d.items() if k != "aux_outputs"} for d in pending],
                                            targets))
        with_indices = lambda d: d if "indices" in d else dict(d, indices=next(found))      # noqa: E731
        top = with_indices(outputs)
        if "aux_outputs" in outputs:
            top = dict(top, aux_outputs=[with_indices(d) for d in aux])
        return previous(self, top, targets)
    return forward


def patch_criterion(criterion_module, matcher_module, *, batch_aux=False, gpu_assignment=False):
    """Opt-in: make the reference's criterion and matchers (``src.models.criterion``, ``src.models.matcher``) run on
    :func:`devis_amd.match_cost` and :func:`devis_amd.box_losses`.  ``DeVISHungarianMatcher.forward`` and
    ``HungarianMatcher.forward`` become one cost call, one device-to-host transfer (cost and status together),
    ``scipy.optimize.linear_sum_assignment`` and index tensors built without a loop over the matches; everything the caller
    sees is the reference's -- values, dtypes, devices, the DeVIS matcher's return after batch element 0 and its triple for a
    clip without targets (no launch).  A degenerate box raises AssertionError and a label outside the classes IndexError,
    from the status.  With ``focal_loss=False`` the replaced method runs.  ``SetCriterion.loss_boxes`` becomes
    :func:`loss_boxes`.  ``SetCriterion.loss_masks`` is not touched (:func:`patch_mask_losses`).

    ``batch_aux=True`` also wraps ``SetCriterion.forward`` (:func:`make_criterion_forward`): the decoder layers' matchings
    share one cost call and one transfer.  The caller's dicts are not mutated.

    ``gpu_assignment=True`` (an opt-in of its own, which combines freely with ``batch_aux``) takes the transfer out of
    ``DeVISHungarianMatcher.forward``: :func:`devis_amd.linear_assignment` solves the cost where it lies and the index
    tensors are formed on the device (:func:`_devis_indices_on_device`), so the matcher neither synchronises nor calls scipy.
    The triples have the reference's values and dtypes, but ``index_i`` and ``index_j`` are on the predictions' device, not on
    the host; the criterion's losses index with them as they are.  Nothing is raised by the matcher: the status counts of both
    operators are left as ``matcher.last_match_status`` for :func:`raise_on_match_status`, to be called where a
    synchronisation is welcome.  A clip without targets, ``focal_loss=False`` and a problem with a side over 1024 take the
    paths described above.  ``HungarianMatcher`` keeps the host path: its consumer reads the indices on the host.  The losses
    after the matcher still synchronise (boolean-mask indexing, ``torch.any``): this removes the matcher's synchronisation only
    (the label loss stops synchronising with :func:`patch_label_loss`).

    Takes effect at once, also for objects that already exist.  Returns what was replaced (to undo the patch;
    :func:`unpatch_criterion`).  The other patches are separate choices."""
    crit, devis, image = criterion_module.SetCriterion, matcher_module.DeVISHungarianMatcher, matcher_module.HungarianMatcher
    previous = {"loss_boxes": crit.loss_boxes, "devis_forward": devis.forward, "image_forward": image.forward}
    if batch_aux:
        previous["criterion_forward"] = crit.forward
    crit.loss_boxes = loss_boxes
    devis.forward = make_matcher_forward(previous["devis_forward"], _devis_indices_on_device if gpu_assignment else _devis_indices)
    image.forward = make_matcher_forward(previous["image_forward"], _image_indices)
    if batch_aux:
        crit.forward = make_criterion_forward(previous["criterion_forward"], {devis: devis.forward, image: image.forward})
    return previous


def unpatch_criterion(criterion_module, matcher_module, previous):
    """Undo :func:`patch_criterion` (tests)."""
    criterion_module.SetCriterion.loss_boxes = previous["loss_boxes"]
    matcher_module.DeVISHungarianMatcher.forward = previous["devis_forward"]
    matcher_module.HungarianMatcher.forward = previous["image_forward"]
    if "criterion_forward" in previous:          # (patched with batch_aux=True)
        criterion_module.SetCriterion.forward = previous["criterion_forward"]


def loss_labels_focal(self, outputs, targets, indices, num_boxes, log=True):
    """A drop-in for the reference's ``SetCriterion.loss_labels_focal`` (``self`` is the criterion) on
    :func:`devis_amd.label_losses`: the matcher's index tensors go to the operator as they lie -- ``rows = cat_i(i * N +
    src_i)``, ``labels = cat_i(targets[i]["labels"][J_i])`` (an integer gather) and, for DeVIS's ``(src, tgt, mask)``
    triples, ``valid = cat_i(mask_i)`` as a tensor, where the reference indexes with the boolean mask and synchronises; image
    matchings ``(src, tgt)`` have no mask.  Index tensors on the host are moved to the logits' device without a synchronising
    copy.  With device indices (``patch_criterion(gpu_assignment=True)``) nothing here synchronises.  Returns ``{"loss_ce"}``
    and, with ``log``, ``"class_error"``.  A match whose row or label is out of range is ignored, not raised on: the
    operator's ``counts[2:]`` tell (:func:`devis_amd.label_loss_terms`)."""
    from . import ops
    assert 'pred_logits' in outputs
    src_logits = outputs['pred_logits']
    N = src_logits.shape[1]
    here = lambda t: t if t.device == src_logits.device else _on_device_of(t, src_logits)      # noqa: E731
    rows = torch.cat([here(entry[0]) + i * N for i, entry in enumerate(indices)])
    labels = torch.cat([here(t["labels"])[here(entry[1])] for t, entry in zip(targets, indices)]).long()
    valid = torch.cat([here(entry[2]) for entry in indices]) if len(indices[0]) == 3 else None
    return ops.label_losses(src_logits, rows.long(), labels, valid, num_boxes, alpha=self.focal_alpha, log=log)


def patch_label_loss(criterion_module):
    """Opt-in: make the reference's criterion (``src.models.criterion``) compute its label loss with
    :func:`loss_labels_focal` -- the fused HIP operator instead of boolean-mask indexing, a one-hot tensor,
    sigmoid_focal_loss and accuracy.  Takes effect at once, also for criteria that already exist (the method is looked up on
    the class).  Returns the replaced function (to undo the patch; :func:`unpatch_label_loss`).  The other patches are
    separate choices."""
    previous = criterion_module.SetCriterion.loss_labels_focal
    criterion_module.SetCriterion.loss_labels_focal = loss_labels_focal
    return previous


def unpatch_label_loss(criterion_module, previous):
    """Undo :func:`patch_label_loss` (tests)."""
    criterion_module.SetCriterion.loss_labels_focal = previous


def _fusable(self, masks, pos_embeds):
    """The position-encoding module all of ``pos_embeds`` were deferred by, when one :func:`devis_amd.encoder_position_embedding`
    call gives what the reference computes from them: every level deferred by the same module from that level's own mask, with
    the same ``.to(dtype)``, and dtypes the kernels write.  None otherwise."""
    from .modules.position_encoding import DeferredPositionEmbedding
    from .functions.position_embedding import OUT_DTYPES
    if not pos_embeds or not all(isinstance(p, DeferredPositionEmbedding) for p in pos_embeds):
        return None
    first = pos_embeds[0]
    for p, m in zip(pos_embeds, masks):
        same_mask = p.mask is m or (p.mask.data_ptr() == m.data_ptr() and p.mask.shape == m.shape and p.mask.stride() == m.stride())
        if p.module is not first.module or p.dtype != first.dtype or not same_mask or p._tensor is not None:
            return None
    temporal_embed = getattr(first.module, "temporal_embed", None)
    if first.dtype not in (None,) + OUT_DTYPES or self.level_embed.dtype not in OUT_DTYPES or \
            (temporal_embed is not None and temporal_embed.dtype not in OUT_DTYPES) or first.module.num_pos_feats % 2:
        return None
    return first.module


def prepare_data_deferred(self, srcs, masks, pos_embeds):
    """``DeformableTransformer.prepare_data`` under :func:`patch_position_encoding` (same arguments, same six results).  When
    every level's position embedding is a :class:`devis_amd.DeferredPositionEmbedding` of one module, ``lvl_pos_embed_flatten``,
    ``mask_flatten`` and ``valid_ratios`` come from ONE :func:`devis_amd.encoder_position_embedding` call -- the per-level
    ``[N, C, H, W]`` tensors, their ``.to(dtype)``, transposes, ``+ level_embed`` and ``cat`` never run --; otherwise the
    deferred ones are materialised and :func:`prepare_data` takes over.  ``spatial_shapes`` / ``level_start_index`` come from
    :func:`interned_pyramid` either way."""
    from . import ops
    from .modules.position_encoding import DeferredPositionEmbedding
    module = _fusable(self, masks, pos_embeds)
    if module is None:
        return prepare_data(self, srcs, masks, [p.materialize() if isinstance(p, DeferredPositionEmbedding) else p for p in pos_embeds])
    dtype = pos_embeds[0].dtype
    src_flatten = flatten_sources(srcs)
    lvl_pos_embed_flatten, mask_flatten, valid_ratios = ops.encoder_position_embedding(
        list(masks), self.level_embed[:len(masks)], getattr(module, "temporal_embed", None), num_pos_feats=module.num_pos_feats,
        temperature=module.temperature, normalize=module.normalize, scale=module.scale if module.normalize else None,
        round_dtype=None if dtype in (None, torch.float32) else dtype)
    spatial_shapes, level_start_index = interned_pyramid([src.shape[-2:] for src in srcs], src_flatten.device)
    return src_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index, valid_ratios


def patch_position_encoding(position_encoding_module, deformable_transformer_module):
    """Opt-in, EAGER ONLY (a :class:`devis_amd.DeferredPositionEmbedding` is a Python object, not a tensor: a traced or compiled
    model calls :func:`devis_amd.encoder_position_embedding` itself): make the forward of the reference's
    ``PositionEmbeddingSine`` and ``PositionEmbeddingSineWithLearnableTemporal`` (``src.models.position_encoding``) return a
    deferred embedding, and ``DeformableTransformer.prepare_data`` (``src.models.deformable_transformer``)
    :func:`prepare_data_deferred`, which computes the encoder's positional input with one fused operator call.

    Order with :func:`patch_transformer`: call ``patch_transformer`` FIRST and this patch second, and the fused
    ``prepare_data`` is the installed one.  In the other order ``patch_transformer`` puts its own ``prepare_data`` over the
    fused one: results are still right -- the deferred embeddings materialise on their first use, through the ``[N, C, H, W]``
    kernel -- but nothing is fused.  Undo in the reverse order of patching.

    Takes effect at once, also for modules that already exist.  Returns what was replaced (to undo the patch;
    :func:`unpatch_position_encoding`).  The other patches are separate choices."""
    from .modules.position_encoding import deferred_forward
    sine = position_encoding_module.PositionEmbeddingSine
    temporal = position_encoding_module.PositionEmbeddingSineWithLearnableTemporal
    top = deformable_transformer_module.DeformableTransformer
    previous = {"sine_forward": sine.__dict__.get("forward"), "temporal_forward": temporal.__dict__.get("forward"),
                "prepare_data": top.__dict__.get("prepare_data")}
    sine.forward = deferred_forward
    temporal.forward = deferred_forward
    top.prepare_data = prepare_data_deferred
    return previous


def unpatch_position_encoding(position_encoding_module, deformable_transformer_module, previous):
    """Undo :func:`patch_position_encoding` (tests)."""
    for cls, name, key in ((position_encoding_module.PositionEmbeddingSine, "forward", "sine_forward"),
                           (position_encoding_module.PositionEmbeddingSineWithLearnableTemporal, "forward", "temporal_forward"),
                           (deformable_transformer_module.DeformableTransformer, "prepare_data", "prepare_data")):
        if previous[key] is None:           # (the class inherited it)
            if name in cls.__dict__:
                delattr(cls, name)
        else:
            setattr(cls, name, previous[key])


def patch_transformer_layers(deformable_transformer_module):
    """Opt-in: make ``forward`` and ``forward_ffn`` of the reference's ``DeformableTransformerEncoderLayer`` and
    ``DeformableTransformerDecoderLayer`` (``src.models.deformable_transformer``; the DeVIS subclasses inherit both) run every
    ``x = norm(x + dropout(y))`` as one :func:`devis_amd.add_layer_norm` call and the FFN as
    ``linear2(relu_dropout(linear1(x)))`` (:mod:`devis_amd.modules.transformer_layers`, which lists when the replaced methods run
    instead: while compiling, on the CPU, with another activation than relu, ...).  Takes effect at once, also for layers that
    already exist (the methods are looked up on the class); no module is replaced, so state dicts are untouched.  Independent of
    every other patch, in either order: :func:`patch_transformer` touches other classes.  Returns what was replaced (to undo the
    patch; :func:`unpatch_transformer_layers`)."""
    from .modules import transformer_layers
    return transformer_layers.patch(deformable_transformer_module)


def unpatch_transformer_layers(deformable_transformer_module, previous):
    """Undo :func:`patch_transformer_layers` (tests)."""
    from .modules import transformer_layers
    transformer_layers.unpatch(deformable_transformer_module, previous)


def patch_self_attention(root_module, *, discard_weights=True):
    """Opt-in: every module under ``root_module`` whose type is exactly ``nn.MultiheadAttention`` -- the ``self_attn`` of the
    reference's ``DeformableTransformerDecoderLayer`` -- becomes a :class:`devis_amd.modules.FusedMultiheadAttention` by setting
    its ``__class__`` (:mod:`devis_amd.modules.self_attention`, which lists when the stock forward runs instead: while compiling,
    on the CPU, with a mask, ...).  No module is replaced: state dicts are untouched and ``copy.deepcopy`` keeps the class;
    subclasses of ``nn.MultiheadAttention`` are left alone.  ``discard_weights=True`` is a stated deviation: a fused call with
    ``need_weights=True`` returns ``None`` where torch returns the head-averaged weights (the reference throws them away); with
    ``discard_weights=False`` such calls run the stock forward.  Independent of :func:`patch_transformer_layers`, in either
    order.  Returns what :func:`unpatch_self_attention` needs."""
    from .modules import self_attention
    return self_attention.patch(root_module, discard_weights)


def unpatch_self_attention(previous):
    """Undo :func:`patch_self_attention`."""
    from .modules import self_attention
    self_attention.unpatch(previous)


def patch_window_attention(swin_backbone_module):
    """Opt-in: make ``forward`` of the reference's ``SwinTransformerBlock`` (``src.models.swin_backbone``) run its cyclic shift,
    window partition, attention with relative-position bias and shift mask, window merge and reverse shift as one
    :func:`devis_amd.window_attention` call between ``self.attn.qkv`` and ``self.attn.proj``
    (:mod:`devis_amd.modules.window_attention`, which lists when the replaced forward runs instead: while compiling, on the CPU,
    in float64, with attention dropout in training, with a window or head dimension the kernels do not take).  The
    ``mask_matrix`` argument is accepted and not read.  Takes effect at once, also for blocks that already exist (the method is
    looked up on the class) and under ``use_checkpoint``; no module is replaced, so state dicts are untouched.  Independent of
    every other patch.  Returns what was replaced (:func:`unpatch_window_attention`)."""
    from .modules import window_attention
    return window_attention.patch(swin_backbone_module)


def unpatch_window_attention(swin_backbone_module, previous):
    """Undo :func:`patch_window_attention`."""
    from .modules import window_attention
    window_attention.unpatch(swin_backbone_module, previous)


def patch_swin_glue(swin_backbone_module):
    """Opt-in: make ``forward`` of the reference's ``SwinTransformerBlock``, ``BasicLayer`` and ``PatchMerging``
    (``src.models.swin_backbone``) run the glue around their Linears and the window attention on the fused kernels of
    :func:`devis_amd.residual_layer_norm` and :func:`devis_amd.patch_merge_norm` (:mod:`devis_amd.modules.swin_glue`, which lists
    when the replaced forwards run instead): ``norm1`` with the copy into the padded window map, the shortcut add with its
    drop-path scale and ``norm2``, a block's last add folded into the next block's first pass, no shift mask, and the patch
    gather with its norm.  The fused blocks call :func:`devis_amd.window_attention` themselves, whether
    :func:`patch_window_attention` is applied or not; where a block is not fusable the forward installed before this patch
    runs.  Takes effect at once, also for modules that already exist; no module is replaced, so state dicts are untouched.
    Returns what was replaced (:func:`unpatch_swin_glue`); undo patches of one module in the reverse of the order they were
    applied in."""
    from .modules import swin_glue
    return swin_glue.patch(swin_backbone_module)


def unpatch_swin_glue(swin_backbone_module, previous):
    """Undo :func:`patch_swin_glue`."""
    from .modules import swin_glue
    swin_glue.unpatch(swin_backbone_module, previous)


def patch_swin_ends(swin_backbone_module):
    """Opt-in: make ``forward`` of the reference's ``PatchEmbed`` and ``SwinTransformer`` (``src.models.swin_backbone``) run the
    entry and the exits of the backbone on the fused kernels of :func:`devis_amd.patch_embed_norm` and
    :func:`devis_amd.layer_norm_to_map` (:mod:`devis_amd.modules.swin_ends`, which lists when the replaced forwards run instead):
    padding, patch projection and norm as one pass into token order -- returned as the reference's NCHW-shaped view, which the
    backbone flattens back without a copy --, and each output norm as one pass into the NCHW map.  Takes effect at once, also for
    modules that already exist; no module is replaced, so state dicts are untouched.  Independent of
    :func:`patch_window_attention` and :func:`patch_swin_glue`, in any order.  Returns what was replaced
    (:func:`unpatch_swin_ends`); undo patches of one module in the reverse of the order they were applied in."""
    from .modules import swin_ends
    return swin_ends.patch(swin_backbone_module)


def unpatch_swin_ends(swin_backbone_module, previous):
    """Undo :func:`patch_swin_ends`."""
    from .modules import swin_ends
    swin_ends.unpatch(swin_backbone_module, previous)


def patch_resnet_glue(module, keep_input_dtype=False):
    """Opt-in: make the blocks and the stem of a ResNet with frozen BatchNorm under ``module`` -- a torchvision ``ResNet``, the
    reference's ``Backbone`` or ``Joiner`` (``src.models.backbone``) or the ``IntermediateLayerGetter`` inside -- run everything
    between their convolutions on the fused kernels of :func:`devis_amd.frozen_batch_norm` and
    :func:`devis_amd.frozen_batch_norm_relu_pool` (:mod:`devis_amd.modules.resnet_glue`, which says what matches, by structure,
    and when the forward a block had runs instead): one call per convolution, the ``downsample`` branch's norm folded into the
    block's tail, and the stem's norm, ReLU and max-pool as one pass.  Instances get a subclass of their own class; no module is
    replaced, so state dicts and ``named_parameters`` are untouched and checkpoints load as before.
    ``keep_input_dtype=True`` is a stated deviation: every fused output takes the dtype of the convolution output it reads
    (16-bit throughout under autocast) where the stock modules return float32.  Returns what :func:`unpatch_resnet_glue` needs."""
    from .modules import resnet_glue
    return resnet_glue.patch(module, keep_input_dtype)


def unpatch_resnet_glue(module, previous):
    """Undo :func:`patch_resnet_glue`."""
    from .modules import resnet_glue
    resnet_glue.unpatch(module, previous)


def patch_input_proj(model):
    """Opt-in, EAGER ONLY (a :class:`devis_amd.DeferredInputProjection` is a Python object, not a tensor): make the ``GroupNorm``
    of every ``Sequential(Conv2d, GroupNorm)`` in ``model.input_proj`` -- the reference's ``DeformableDETR``
    (``src.models.deformable_detr``), or anything with such a ``ModuleList`` -- return a deferred projection, which
    :func:`prepare_data` and :func:`prepare_data_deferred` turn into ``src_flatten`` with one fused
    :func:`devis_amd.group_norm_tokens` call for all levels (:mod:`devis_amd.modules.input_projection`).  A 3 x 3 / stride-2
    projection that is followed by another one (five or more levels) feeds the next convolution and is not deferred: it runs
    the one-level kernel at once.  The ``GroupNorm`` instances get a subclass; no module is replaced, so state dicts are
    untouched.

    Order: the fused path needs one of this package's ``prepare_data`` -- call :func:`patch_transformer` (and, for the fused
    positional input, :func:`patch_position_encoding` after it) as well, in any order relative to this patch.  Under the stock
    ``prepare_data`` the deferred projections materialise on ``.flatten(2)``, level by level through the one-level kernel:
    results are right and nothing is fused.  Independent of every other patch.  Returns what :func:`unpatch_input_proj` needs."""
    from .modules import input_projection
    return input_projection.patch(model)


def unpatch_input_proj(model, previous):
    """Undo :func:`patch_input_proj`."""
    from .modules import input_projection
    input_projection.unpatch(model, previous)

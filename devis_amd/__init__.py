"""devis_amd -- MI355X-native (gfx950 / CDNA4) multi-scale deformable attention and deformable convolution for DeVIS.

A from-scratch replacement for DeVIS's native components: ``src/models/ops`` (the vendored
Deformable-DETR CUDA extension ``MultiScaleDeformableAttention`` plus its Python wrappers), behind the
same Python surface::

    from devis_amd.functions import MSDeformAttnFunction, ms_deform_attn_core_pytorch
    from devis_amd.modules import MSDeformAttn, TemporalMSDeformAttnEncoder, TemporalMSDeformAttnDecoder

and the mask head's ``torchvision.ops.deform_conv2d`` (``devis_amd.deform_conv2d``, same signature; the module
``devis_amd.modules.ModulatedDeformableConv2d``; C ABI ``include/mdcn.h``) and its attention maps
(``devis_amd.attention_maps``; the module ``devis_amd.modules.MultiScaleMHAttentionMap``; C ABI ``include/attmap.h``) and the
glue between its convolutions (``devis_amd.mask_head_stage``; the module ``devis_amd.modules.MaskHeadConv``; C ABI
``include/mhstage.h``) and the mask loss of its criterion (``devis_amd.mask_losses``; C ABI ``include/maskloss.h``) and the clip stitching of its tracker
(``devis_amd.mask_soft_iou``, ``devis_amd.binarize_masks``; C ABI ``include/maskiou.h``) and the run lengths its mask
encoder counts (``devis_amd.mask_run_lengths``; C ABI ``include/maskrle.h``) and the binary mask IoU of its other stitching
mode (``devis_amd.mask_binary_iou``, ``devis_amd.mask_binary_iou_terms``; C ABI ``include/maskbiou.h``) and the matching cost
and box losses of its criterion (``devis_amd.match_cost``, ``devis_amd.box_losses``; C ABI ``include/boxmatch.h``) and the
assignment its matchers make of that cost (``devis_amd.linear_assignment``; C ABI ``include/assign.h``) and the label loss of
its criterion (``devis_amd.label_losses``; C ABI ``include/labelloss.h``) and the positional input of its encoder
(``devis_amd.encoder_position_embedding``, ``devis_amd.sine_position_embedding``; the modules
``devis_amd.modules.PositionEmbeddingSine`` / ``PositionEmbeddingSineWithLearnableTemporal``; C ABI ``include/posembed.h``) and the glue between the GEMMs of its transformer
layers -- residual, dropout and LayerNorm, and the FFN's relu and dropout (``devis_amd.add_layer_norm``,
``devis_amd.relu_dropout``, ``devis_amd.patch_transformer_layers``; C ABI ``include/addnorm.h``) and the query self-attention
of its decoder layers between the projections of ``nn.MultiheadAttention`` (``devis_amd.multihead_attention``; the module
``devis_amd.modules.FusedMultiheadAttention``; ``devis_amd.patch_self_attention``; C ABI ``include/selfattn.h``) and the
(shifted-)window attention of its Swin backbone between the ``qkv`` and ``proj`` Linears of a ``SwinTransformerBlock``
(``devis_amd.window_attention``; ``devis_amd.patch_window_attention``; C ABI ``include/winattn.h``) and the glue around
that attention and the blocks' Linears -- the residual add with its drop-path scale, the pre-norm LayerNorm written into the
zero-padded window map, and the patch merge's gather with its norm (``devis_amd.residual_layer_norm``,
``devis_amd.patch_merge_norm``; ``devis_amd.patch_swin_glue``; C ABI ``include/prenorm.h``) and the two ends of that backbone -- the patch embedding with
its norm written in token order and the per-stage output norms written as NCHW maps (``devis_amd.patch_embed_norm``,
``devis_amd.layer_norm_to_map``; ``devis_amd.patch_swin_ends``; C ABI ``include/swinends.h``) and the glue between the
convolutions of its ResNet backbone -- the frozen BatchNorm's affine map with the ReLU, the shortcut add with the downsample
branch's norm folded in, and the stem's max-pool (``devis_amd.frozen_batch_norm``, ``devis_amd.frozen_batch_norm_relu_pool``;
``devis_amd.patch_resnet_glue``; C ABI ``include/frozennorm.h``) and the seam between the backbone and the encoder -- the
GroupNorm of every input projection written once as the encoder's flat token tensor ``src_flatten``
(``devis_amd.group_norm_tokens``; ``devis_amd.patch_input_proj``; C ABI ``include/inputproj.h``).

Arithmetic lives in hand-written HIP kernels behind the C ABI of ``include/msda.h``
(``devis_amd/csrc/*.hip``, one translation unit per kernel family -> ``devis_amd/libmsda_hip.so``); the Python here is the host side.
Under ``torch.compile`` and ``torch.export`` the same host code runs as the custom ops of :mod:`devis_amd.ops`.
There is no CPU fallback: like the reference (``src/ms_deform_attn.h:38,60``) the operator raises on
CPU tensors, and it raises if the HIP library cannot be loaded.
"""
from .functions import (MSDeformAttnFunction, MSDeformAttnTemporalFunction,  # noqa: F401
                        ms_deform_attn_core_pytorch)
from .modules import (MaskHeadConv, ModulatedDeformableConv2d, MSDeformAttn, MultiScaleMHAttentionMap,  # noqa: F401
                      TemporalMSDeformAttnDecoder, TemporalMSDeformAttnEncoder)
from . import ops  # noqa: F401  (the operator as torch.library custom ops: torch.compile / torch.export)
from .ops import attention_maps, deform_conv2d, mask_head_stage, mask_loss_terms, mask_losses  # noqa: F401
from .ops import binarize_masks, mask_run_lengths, mask_soft_iou, mask_soft_iou_terms  # noqa: F401
from .ops import mask_binary_iou, mask_binary_iou_terms  # noqa: F401
from .ops import box_loss_terms, box_losses, match_cost  # noqa: F401
from .ops import linear_assignment  # noqa: F401
from .ops import label_loss_terms, label_losses  # noqa: F401
from .ops import encoder_position_embedding, sine_position_embedding  # noqa: F401
from .modules.position_encoding import DeferredPositionEmbedding  # noqa: F401
from .functions.deform_conv import reproducible_grad_input, reproducible_grad_input_enabled  # noqa: F401
from .argument_builders import patch_attention_maps, patch_mask_head, patch_transformer, unpatch_attention_maps  # noqa: F401
from .argument_builders import patch_mask_head_stages, unpatch_mask_head_stages  # noqa: F401
from .argument_builders import patch_mask_losses, unpatch_mask_losses  # noqa: F401
from .argument_builders import patch_tracker, unpatch_tracker  # noqa: F401
from .argument_builders import patch_criterion, raise_on_match_status, unpatch_criterion  # noqa: F401
from .argument_builders import patch_label_loss, unpatch_label_loss  # noqa: F401
from .argument_builders import patch_position_encoding, unpatch_position_encoding  # noqa: F401
from .argument_builders import patch_transformer_layers, unpatch_transformer_layers  # noqa: F401
from .functions.add_norm import add_layer_norm, relu_dropout  # noqa: F401  (eager kernels; the torch composite while compiling)
from .argument_builders import patch_self_attention, unpatch_self_attention  # noqa: F401
from .functions.self_attention import multihead_attention  # noqa: F401  (eager kernels; the torch composite while compiling)
from .modules import FusedMultiheadAttention  # noqa: F401
from .argument_builders import patch_window_attention, unpatch_window_attention  # noqa: F401
from .functions.window_attention import window_attention  # noqa: F401  (eager kernels; the torch composite while compiling)
from .argument_builders import patch_swin_glue, unpatch_swin_glue  # noqa: F401
from .functions.pre_norm import patch_merge_norm, residual_layer_norm  # noqa: F401  (eager kernels; the torch composite while compiling)
from .argument_builders import patch_swin_ends, unpatch_swin_ends  # noqa: F401
from .functions.swin_ends import layer_norm_to_map, patch_embed_norm  # noqa: F401  (eager kernels; the torch composite while compiling)
from .argument_builders import patch_resnet_glue, unpatch_resnet_glue  # noqa: F401
from .argument_builders import patch_input_proj, unpatch_input_proj  # noqa: F401
from .functions.input_projection import group_norm_tokens  # noqa: F401  (eager kernels; the torch composite while compiling)
from .modules.input_projection import DeferredInputProjection  # noqa: F401
from .functions.frozen_norm import frozen_batch_norm, frozen_batch_norm_relu_pool  # noqa: F401  (eager kernels; the torch composite while compiling)
from .tracking import LogitMask  # noqa: F401
from .graphs import graphed, graph_stream, GraphedLayer  # noqa: F401
from .tuning import tune  # noqa: F401

__all__ = ["MSDeformAttnFunction", "MSDeformAttnTemporalFunction", "ms_deform_attn_core_pytorch",
           "MSDeformAttn", "TemporalMSDeformAttnEncoder", "TemporalMSDeformAttnDecoder", "ModulatedDeformableConv2d", "MultiScaleMHAttentionMap", "deform_conv2d", "attention_maps", "patch_attention_maps", "unpatch_attention_maps", "mask_head_stage", "MaskHeadConv", "patch_mask_head_stages", "unpatch_mask_head_stages", "mask_loss_terms", "mask_losses", "patch_mask_losses", "unpatch_mask_losses", "mask_soft_iou", "mask_soft_iou_terms", "binarize_masks", "mask_run_lengths", "mask_binary_iou", "mask_binary_iou_terms", "LogitMask", "patch_tracker", "unpatch_tracker", "match_cost", "box_loss_terms", "box_losses", "patch_criterion", "unpatch_criterion", "linear_assignment", "raise_on_match_status", "label_loss_terms", "label_losses", "patch_label_loss", "unpatch_label_loss", "sine_position_embedding", "encoder_position_embedding", "DeferredPositionEmbedding", "patch_position_encoding", "unpatch_position_encoding", "add_layer_norm", "relu_dropout", "patch_transformer_layers", "unpatch_transformer_layers", "multihead_attention", "FusedMultiheadAttention", "patch_self_attention", "unpatch_self_attention", "window_attention", "patch_window_attention", "unpatch_window_attention", "residual_layer_norm", "patch_merge_norm", "patch_swin_glue", "unpatch_swin_glue", "patch_embed_norm", "layer_norm_to_map", "patch_swin_ends", "unpatch_swin_ends", "frozen_batch_norm", "frozen_batch_norm_relu_pool", "patch_resnet_glue", "unpatch_resnet_glue", "group_norm_tokens", "DeferredInputProjection", "patch_input_proj", "unpatch_input_proj", "reproducible_grad_input", "reproducible_grad_input_enabled", "ops", "patch_transformer", "patch_mask_head", "graphed", "graph_stream", "GraphedLayer", "tune"]

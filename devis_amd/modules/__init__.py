# mirrors /root/reference/src/models/ops/modules/__init__.py:9 (same exported names)
from .ms_deform_attn import (MSDeformAttn, TemporalMSDeformAttnBase,  # noqa: F401
                             TemporalMSDeformAttnDecoder, TemporalMSDeformAttnEncoder)
from .deform_conv import ModulatedDeformableConv2d  # noqa: F401  (reference src/models/deformable_segmentation.py)
from .attention_maps import MultiScaleMHAttentionMap  # noqa: F401  (reference src/models/deformable_segmentation.py)
from .mask_head import MaskHeadConv  # noqa: F401  (reference src/models/deformable_segmentation.py)
from .position_encoding import (PositionEmbeddingSine,  # noqa: F401  (reference src/models/position_encoding.py)
                                PositionEmbeddingSineWithLearnableTemporal)
from .self_attention import FusedMultiheadAttention  # noqa: F401  (reference src/models/deformable_transformer.py: self_attn)

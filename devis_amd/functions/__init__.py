# mirrors /root/reference/src/models/ops/functions/__init__.py:9 (same exported names)
from .ms_deform_attn_func import (MSDeformAttnFunction, MSDeformAttnTemporalFunction,  # noqa: F401
                                  ms_deform_attn_core_pytorch, project_value,
                                  MSDeformPrepFunction, MSDeformPrepFusedFunction)
from .attention_maps import AttentionMapsFunction  # noqa: F401  (the mask head's attention maps: include/attmap.h)
from .mask_head_stage import MaskHeadStageFunction  # noqa: F401  (one stage of the mask head's glue: include/mhstage.h)
from .mask_losses import MaskLossTermsFunction  # noqa: F401  (the mask loss: include/maskloss.h)

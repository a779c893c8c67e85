"""Run config and result of the char-mask engines (reference: engine/char_mask/type.py)."""
from typing import Optional, Sequence

import attrs

from vkit_amd.element import Box, Mask, Polygon


@attrs.define
class CharMaskEngineRunConfig:
    height: int
    width: int
    char_polygons: Sequence[Polygon]
    char_bounding_boxes: Optional[Sequence[Box]] = None
    char_bounding_polygons: Optional[Sequence[Polygon]] = None


@attrs.define
class CharMask:
    combined_chars_mask: Mask
    char_masks: Optional[Sequence[Mask]] = None
